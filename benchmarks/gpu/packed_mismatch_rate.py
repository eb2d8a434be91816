"""fmx_mismatch_hits_batch_packed2_dev / ..._rc_dev (one pass into max_hits slots per pattern) against the byte call of the
same session -- fmx_mismatch_count_batch_dev + fmx_offsets_dev + fmx_mismatch_search_batch_dev on the byte form of the
batch, and for both strands on the 2 N virtual batch with reverse complements made before anything is timed -- on the
config-2 DNA text (fm_index_amd.workload.dna_text_torch, seed 1), patterns resident on the device.  Pass 1 of the byte
call alone is recorded too: the floor the one-pass kernel is expected to sit near.

Two indexes of the same text (the default one and plain=True), two pattern sets (substrings with one symbol changed at a
uniform position; uniform random patterns), K = 1 on --npat patterns and K = 2 on --npat2.  Before anything is timed
every result of the new calls is compared with the byte call's: nint, count, and the first min(nint, max_hits) intervals
and edits of every (virtual) pattern; the rest of the slots must hold the filler.  Times are HIP-event times per call (mean
of --steps back-to-back calls), median of --runs runs; --out is rewritten with one JSON line per (index, K, set).
    python benchmarks/gpu/packed_mismatch_rate.py --out profiles/r16/packed_mismatch.jsonl"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.getcwd())
import torch

import fm_index_amd as F
from fm_index_amd import _lib as L
from fm_index_amd import workload as W

ap = argparse.ArgumentParser()
ap.add_argument("--log2n", type=int, default=30)
ap.add_argument("--npat", type=int, default=1 << 20)
ap.add_argument("--npat2", type=int, default=1 << 16)
ap.add_argument("--max-hits", type=int, default=4)
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--out", default="profiles/r16/packed_mismatch.jsonl")
args = ap.parse_args()

dev = torch.device("cuda", 0)
torch.cuda.set_device(0)
lib = L.lib()
n, m, mh = 1 << args.log2n, 32, args.max_hits         # 32 symbols: a pattern is one word of the packed stream
text = W.dna_text_torch(n, 1, dev)
stream = torch.cuda.current_stream()
sp = C.c_void_p(stream.cuda_stream)
ALL = -1                                              # UINT64_MAX as torch sees it


def P(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def check(rc):
    if rc != 0:
        raise RuntimeError(lib.fmx_last_error().decode())


def event_ms(fn, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(steps):
        fn()
    e1.record(stream)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def med(fn):
    fn()
    torch.cuda.synchronize()
    xs = [event_ms(fn, args.steps) for _ in range(args.runs)]
    return {"median_ms": round(statistics.median(xs), 4), "min_ms": round(min(xs), 4), "max_ms": round(max(xs), 4)}


def pattern_sets(npat):
    src = W.umod_torch(W.splitmix64_torch(3, 0, npat, dev), n - 1 - m)
    sub = text[src[:, None] + torch.arange(m, dtype=torch.int64, device=dev)[None, :]].contiguous()
    where = W.umod_torch(W.splitmix64_torch(11, 0, npat, dev), m)
    bump = W.umod_torch(W.splitmix64_torch(12, 0, npat, dev), 3) + 1                # 1..3: always another symbol
    changed = sub.clone()
    rows = torch.arange(npat, device=dev)
    changed[rows, where] = ((changed[rows, where].to(torch.int64) - 1 + bump) % 4 + 1).to(torch.uint8)
    rnd = (W.umod_torch(W.splitmix64_torch(13, 0, npat * m, dev), 4) + 1).to(torch.uint8).view(npat, m).contiguous()
    return {"one_changed": changed, "random": rnd}


class ByteCall:
    """the yardstick on an (N, m) u8 batch: pass 1, the scan, pass 2; its arrays allocated before anything is timed"""

    def __init__(self, h, pat2d, K):
        self.h, self.K, self.N, self.flat = h, K, pat2d.shape[0], pat2d.reshape(-1).contiguous()
        self.off = (torch.arange(self.N + 1, dtype=torch.int64, device=dev) * m).contiguous()
        self.n, self.c, self.zero = (torch.zeros(self.N, dtype=torch.int64, device=dev) for _ in range(3))
        self.oo = torch.zeros(self.N + 1, dtype=torch.int64, device=dev)
        self.pass1()
        self.scan()
        torch.cuda.synchronize()
        self.total = int(self.oo[-1].item())
        self.s, self.e = (torch.empty(max(self.total, 1), dtype=torch.int64, device=dev) for _ in range(2))
        self.ed = torch.empty(2 * max(self.total, 1), dtype=torch.int64, device=dev)

    def pass1(self):
        check(lib.fmx_mismatch_count_batch_dev(self.h, P(self.flat), P(self.off), self.N, None, self.K, P(self.n),
                                               P(self.c), sp))

    def scan(self):
        check(lib.fmx_offsets_dev(self.h, P(self.zero), P(self.n), self.N, P(self.oo), sp))

    def whole(self):
        self.pass1()
        self.scan()
        check(lib.fmx_mismatch_search_batch_dev(self.h, P(self.flat), P(self.off), self.N, None, self.K, P(self.oo),
                                                self.total, P(self.s), P(self.e), P(self.ed), sp))


class PackedCall:
    def __init__(self, h, words, npat, K, both):
        self.h, self.K, self.npat, self.words = h, K, npat, words
        self.fn = lib.fmx_mismatch_hits_batch_packed2_rc_dev if both else lib.fmx_mismatch_hits_batch_packed2_dev
        self.off = (torch.arange(npat + 1, dtype=torch.int64, device=dev) * m).contiguous()
        nv = npat * (2 if both else 1)
        self.n, self.c = (torch.zeros(nv, dtype=torch.int64, device=dev) for _ in range(2))
        self.s, self.e = (torch.full((nv, mh), 7, dtype=torch.int64, device=dev) for _ in range(2))
        self.ed = torch.full((nv, mh, 2), 7, dtype=torch.int64, device=dev)

    def whole(self):
        check(self.fn(self.h, P(self.words), P(self.off), self.npat, self.K, mh, P(self.n), P(self.c), P(self.s),
                      P(self.e), P(self.ed), sp))

    def agrees_with(self, b):
        j = torch.arange(mh, device=dev)[None, :]
        used = j < self.n[:, None]
        at = (b.oo[:-1, None] + j).clamp(max=max(b.total, 1) - 1)
        ok = bool((self.n == b.n).all()) and bool((self.c == b.c).all())
        ok = ok and bool((self.s == torch.where(used, b.s[at], 0)).all()) and bool((self.e == torch.where(used, b.e[at], 0)).all())
        for t in (0, 1):
            ok = ok and bool((self.ed[:, :, t] == torch.where(used, b.ed[2 * at + t], ALL)).all())
        return ok


os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
open(args.out, "w").close()                           # a run replaces the file
work = [(1, args.npat), (2, args.npat2)]
sets_by_npat = {npat: pattern_sets(npat) for _, npat in work}
shifts = (torch.arange(m, dtype=torch.int64, device=dev) * 2)[None, :]
for iname, kw in (("plain", {"plain": True}), ("default", {})):
    index = F.FMIndex.from_device_text(text.data_ptr(), n, 4, device=0, **kw)
    h = index.handle()
    for K, npat in work:
        for sname, pat2d in sets_by_npat[npat].items():
            words = ((pat2d.to(torch.int64) - 1) << shifts).sum(dim=1).contiguous()   # disjoint fields: no carry
            virt = torch.stack([pat2d, (5 - pat2d.flip(1)).to(torch.uint8)], dim=1).view(2 * npat, m).contiguous()
            b1, b2 = ByteCall(h, pat2d, K), ByteCall(h, virt, K)
            p1, p2 = PackedCall(h, words, npat, K, False), PackedCall(h, words, npat, K, True)
            for x in (b1, b2, p1, p2):
                x.whole()
            torch.cuda.synchronize()
            assert lib.fmx_stream_status(h) == 0
            assert p1.agrees_with(b1) and p2.agrees_with(b2), "the packed call differs from the byte call"
            rec = {"index": iname, "K": K, "set": sname, "log2n": args.log2n, "npat": npat, "plen": m, "max_hits": mh,
                   "pair_index": index.has_pair_index(), "kmer_k": index.kmer_k(), "steps": args.steps, "runs": args.runs,
                   "intervals_per_pattern": round(b1.total / npat, 4),
                   "intervals_per_virtual_pattern": round(b2.total / (2 * npat), 4),
                   "truncated_share": round(float((p2.n > mh).double().mean().item()), 5),
                   "byte": med(b1.whole), "byte_pass1": med(b1.pass1), "packed": med(p1.whole),
                   "byte_2n": med(b2.whole), "byte_2n_pass1": med(b2.pass1), "both_strands": med(p2.whole)}
            rec["ratio_single"] = round(rec["byte"]["median_ms"] / rec["packed"]["median_ms"], 3)
            rec["ratio_both"] = round(rec["byte_2n"]["median_ms"] / rec["both_strands"]["median_ms"], 3)
            # a leg that is slower than its yardstick by more than the yardstick's own spread
            rec["slower_beyond_spread"] = [leg for leg, y in (("packed", "byte"), ("both_strands", "byte_2n"))
                                           if rec[leg]["median_ms"] > rec[y]["max_ms"]]
            print(json.dumps(rec), flush=True)
            with open(args.out, "a") as f:
                f.write(json.dumps(rec) + "\n")
            del b1, b2, p1, p2, virt, words
    index.close()
