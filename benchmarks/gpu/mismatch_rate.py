"""fmx_mismatch_count_batch_dev + fmx_offsets_dev + fmx_mismatch_search_batch_dev against fmx_count_batch_dev on the same
batch (the floor: K = 0) and against the emulation the call replaces -- fmx_count_batch_dev on every enumerated variant
of every pattern (1 + 3 m at K = 1: 97 for m = 32; 1 + 3 m + 9 m (m - 1) / 2 at K = 2: 4561) -- on the config-2 DNA
text (fm_index_amd.workload.dna_text_torch, seed 1), patterns resident on the device.

Two indexes of the same text (the default one and plain=True), two pattern sets (substrings with one symbol changed at a
uniform position; uniform random patterns), K = 1 on --npat patterns and K = 2 on --npat2.  The emulation runs on
--nemu1 / --nemu2 patterns (its variants are built on the device before anything is timed, its buffers allocated once)
and its time is scaled per pattern.  Before anything is timed its counts are compared with the new call's: per pattern the
sum over the variants is out_count and the number of variants that occur is out_nint.  Times are HIP-event times per call
(mean of --steps back-to-back calls), median of --runs runs; --out is rewritten with one JSON line per (index, K, set).
    python benchmarks/gpu/mismatch_rate.py --out profiles/r10/mismatch.jsonl"""
import argparse
import ctypes as C
import itertools
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
ap.add_argument("--nemu1", type=int, default=1 << 16)
ap.add_argument("--nemu2", type=int, default=1 << 12)
ap.add_argument("--plen", type=int, default=32)
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--out", default="profiles/r10/mismatch.jsonl")
args = ap.parse_args()

dev = torch.device("cuda", 0)
torch.cuda.set_device(0)
lib = L.lib()
n, m = 1 << args.log2n, args.plen
text = W.dna_text_torch(n, 1, dev)
stream = torch.cuda.current_stream()
sp = C.c_void_p(stream.cuda_stream)


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


def med(fn, steps):
    fn()
    torch.cuda.synchronize()
    xs = [event_ms(fn, steps) for _ in range(args.runs)]
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


def all_variants(base, K):
    """(npat, nvar, m) u8: the pattern itself and every variant with 1 .. K symbols replaced by another of 1..4"""
    npat = base.shape[0]
    b = base.to(torch.int64)
    parts = [base[:, None, :]]
    for k in range(1, K + 1):
        combos = list(itertools.combinations(range(m), k))
        deltas = list(itertools.product((1, 2, 3), repeat=k))
        pos = torch.tensor([c for c in combos for _ in deltas], device=dev)          # (nv, k)
        dl = torch.tensor([d for _ in combos for d in deltas], device=dev)           # (nv, k)
        v = base[:, None, :].repeat(1, pos.shape[0], 1)
        ar = torch.arange(pos.shape[0], device=dev)
        for q in range(k):
            v[:, ar, pos[:, q]] = ((b[:, pos[:, q]] - 1 + dl[None, :, q]) % 4 + 1).to(torch.uint8)
        parts.append(v)
    return torch.cat(parts, dim=1).contiguous()


os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
open(args.out, "w").close()                           # a run replaces the file
work = [(1, args.npat, args.nemu1), (2, args.npat2, args.nemu2)]
sets_by_npat = {npat: pattern_sets(npat) for _, npat, _ in work}
for iname, kw in (("plain", {"plain": True}), ("default", {})):
    index = F.FMIndex.from_device_text(text.data_ptr(), n, 4, device=0, **kw)
    h = index.handle()
    for K, npat, nemu in work:
        off = (torch.arange(npat + 1, dtype=torch.int64, device=dev) * m).contiguous()
        d_n, d_c, d_zero = (torch.zeros(npat, dtype=torch.int64, device=dev) for _ in range(3))
        d_oo = torch.zeros(npat + 1, dtype=torch.int64, device=dev)
        c_s, c_e, c_c = (torch.empty(npat, dtype=torch.int64, device=dev) for _ in range(3))
        for sname, pat2d in sets_by_npat[npat].items():
            flat = pat2d.view(-1)

            def pass1():
                check(lib.fmx_mismatch_count_batch_dev(h, P(flat), P(off), npat, None, K, P(d_n), P(d_c), sp))

            def scan():
                check(lib.fmx_offsets_dev(h, P(d_zero), P(d_n), npat, P(d_oo), sp))

            pass1()
            scan()
            torch.cuda.synchronize()
            assert lib.fmx_stream_status(h) == 0
            total = int(d_oo[-1].item())
            d_s, d_e = (torch.empty(max(total, 1), dtype=torch.int64, device=dev) for _ in range(2))
            d_ed = torch.empty(2 * max(total, 1), dtype=torch.int64, device=dev)

            def pass2():
                check(lib.fmx_mismatch_search_batch_dev(h, P(flat), P(off), npat, None, K, P(d_oo), total, P(d_s), P(d_e),
                                                        P(d_ed), sp))

            def whole():
                pass1()
                scan()
                pass2()

            def count_call():
                check(lib.fmx_count_batch_dev(h, P(flat), P(off), npat, None, P(c_s), P(c_e), P(c_c), sp))

            # the emulation: fmx_count_batch_dev on every variant of the first `nemu` patterns
            var = all_variants(pat2d[:nemu], K)
            nvar = var.shape[1]
            vflat = var.view(-1)
            voff = (torch.arange(nemu * nvar + 1, dtype=torch.int64, device=dev) * m).contiguous()
            v_s, v_e, v_c = (torch.empty(nemu * nvar, dtype=torch.int64, device=dev) for _ in range(3))

            def emulation():
                check(lib.fmx_count_batch_dev(h, P(vflat), P(voff), nemu * nvar, None, P(v_s), P(v_e), P(v_c), sp))

            whole()
            emulation()
            torch.cuda.synchronize()
            assert lib.fmx_stream_status(h) == 0
            per = v_c.view(nemu, nvar)
            assert bool((per.sum(dim=1) == d_c[:nemu]).all()) and bool(((per > 0).sum(dim=1) == d_n[:nemu]).all())
            rec = {"index": iname, "K": K, "set": sname, "log2n": args.log2n, "npat": npat, "plen": m,
                   "pair_index": index.has_pair_index(), "kmer_k": index.kmer_k(), "steps": args.steps, "runs": args.runs,
                   "intervals_per_pattern": round(total / npat, 4),
                   "occurrences_per_pattern": round(float(d_c.double().mean().item()), 4),
                   "pass1": med(pass1, args.steps), "pass2": med(pass2, args.steps),
                   "both_passes_and_scan": med(whole, args.steps), "count_same_batch": med(count_call, args.steps),
                   "emulation_npat": nemu, "emulation_variants_per_pattern": nvar,
                   "emulation": med(emulation, max(args.steps // 2, 1))}
            rec["emulation_scaled_ms"] = round(rec["emulation"]["median_ms"] * npat / nemu, 4)
            rec["ratio_to_count"] = round(rec["both_passes_and_scan"]["median_ms"] / rec["count_same_batch"]["median_ms"], 3)
            rec["ratio_emulation_to_call"] = round(rec["emulation_scaled_ms"] / rec["both_passes_and_scan"]["median_ms"], 3)
            print(json.dumps(rec), flush=True)
            with open(args.out, "a") as f:
                f.write(json.dumps(rec) + "\n")
            del var, vflat, voff, v_s, v_e, v_c, d_s, d_e, d_ed
    index.close()
