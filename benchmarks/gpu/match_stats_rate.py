"""fmx_match_stats_batch_dev against the two yardsticks of DESIGN.md section 4.2d, on the config-2 DNA text
(fm_index_amd.workload.dna_text_torch, seed 1) and the three pattern sets of benchmarks/gpu/suffix_match_rate.py
(substrings, one symbol changed, random), `--npat` patterns of `--plen` symbols, all resident on the device:
    (a) the emulation the call replaces: fmx_suffix_match_batch_dev on a copy of EVERY PREFIX of every pattern.  The
        copies (plen times the patterns, (plen + 1) / 2 times the pattern bytes) are built once, outside the timed
        region: the copy pass and that memory come on top of the time reported here.
    (b) fmx_count_batch_dev on the same batch, times plen: the naive lower bound per slot.
The new call is timed with the filter off and with --min-seed-len.  Times are HIP-event times per call (mean of --steps
back-to-back calls), median of --runs runs; --out is rewritten with one JSON line per (index, set).  The emulation's
result is compared with the new call's before anything is timed.
    python benchmarks/gpu/match_stats_rate.py --out profiles/r11/match_stats.jsonl"""
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
ap.add_argument("--plen", type=int, default=32)
ap.add_argument("--min-count", type=int, default=1)
ap.add_argument("--min-seed-len", type=int, default=19)
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--out", default="profiles/r11/match_stats.jsonl")
args = ap.parse_args()

dev = torch.device("cuda", 0)
torch.cuda.set_device(0)
lib = L.lib()
n, npat, m, mc = 1 << args.log2n, args.npat, args.plen, max(args.min_count, 1)
total = npat * m
text = W.dna_text_torch(n, 1, dev)
stream = torch.cuda.current_stream()
sp = C.c_void_p(stream.cuda_stream)


def P(t):
    return None if t is None else C.c_void_p(t.data_ptr())


# ---- the three pattern sets (as in suffix_match_rate.py) ----
src = W.umod_torch(W.splitmix64_torch(3, 0, npat, dev), n - 1 - m)
sub = text[src[:, None] + torch.arange(m, dtype=torch.int64, device=dev)[None, :]].contiguous()
where = W.umod_torch(W.splitmix64_torch(11, 0, npat, dev), m)
bump = W.umod_torch(W.splitmix64_torch(12, 0, npat, dev), 3) + 1                    # 1..3: always another symbol
changed = sub.clone()
rows = torch.arange(npat, device=dev)
changed[rows, where] = ((changed[rows, where].to(torch.int64) - 1 + bump) % 4 + 1).to(torch.uint8)
rnd = (W.umod_torch(W.splitmix64_torch(13, 0, npat * m, dev), 4) + 1).to(torch.uint8).view(npat, m).contiguous()
sets = {"substring": sub, "one_changed": changed, "random": rnd}
off = (torch.arange(npat + 1, dtype=torch.int64, device=dev) * m).contiguous()
d_s, d_e, d_l = (torch.empty(total, dtype=torch.int64, device=dev) for _ in range(3))
c_s, c_e, c_c = (torch.empty(npat, dtype=torch.int64, device=dev) for _ in range(3))
# the emulation's buffers: one pattern per slot, prefix i of pattern k at slot k * m + i - 1
plen = torch.arange(1, m + 1, dtype=torch.int64, device=dev).repeat(npat)
poff = torch.zeros(total + 1, dtype=torch.int64, device=dev)
poff[1:] = torch.cumsum(plen, 0)
del plen
pflat = torch.empty(npat * (m * (m + 1) // 2), dtype=torch.uint8, device=dev)
tri = (torch.arange(m, device=dev)[None, :] < torch.arange(1, m + 1, device=dev)[:, None])          # [i - 1, j]: j < i
e_s, e_e, e_l = (torch.empty(total, dtype=torch.int64, device=dev) for _ in range(3))


def build_prefix_copies(pat2d):
    per, chunk = m * (m + 1) // 2, 1 << 14
    for a in range(0, npat, chunk):
        b = min(a + chunk, npat)
        blk = pat2d[a:b, None, :].expand(b - a, m, m)
        pflat[a * per:b * per] = blk[tri[None, :, :].expand(b - a, m, m)]


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


os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
open(args.out, "w").close()                           # a run replaces the file: one record per (index, set)
for iname, kw in (("default", {}), ("plain", {"plain": True})):
    index = F.FMIndex.from_device_text(text.data_ptr(), n, 4, device=0, **kw)
    h = index.handle()
    for sname, pat2d in sets.items():
        flat = pat2d.view(-1)
        build_prefix_copies(pat2d)

        def stats(msl):
            check(lib.fmx_match_stats_batch_dev(h, P(flat), P(off), npat, total, mc, 0, msl, P(d_s), P(d_e), P(d_l), sp))

        def emulation():
            check(lib.fmx_suffix_match_batch_dev(h, P(pflat), P(poff), total, None, mc, P(e_s), P(e_e), None, P(e_l), sp))

        def count_call():
            check(lib.fmx_count_batch_dev(h, P(flat), P(off), npat, None, P(c_s), P(c_e), P(c_c), sp))

        stats(0)
        emulation()
        torch.cuda.synchronize()
        assert lib.fmx_stream_status(h) == 0
        hit = e_l > 0
        assert bool((e_l == d_l).all()) and bool((e_s[hit] == d_s[hit]).all()) and bool((e_e[hit] == d_e[hit]).all())
        assert not bool(d_s[~hit].any()) and not bool(d_e[~hit].any())
        mean_len = round(float(d_l.double().mean().item()), 3)
        del hit
        stats(args.min_seed_len)
        torch.cuda.synchronize()
        nseeds = int((d_e > d_s).sum().item())
        rec = {"index": iname, "set": sname, "log2n": args.log2n, "npat": npat, "plen": m, "slots": total,
               "min_count": mc, "max_len": 0, "min_seed_len": args.min_seed_len, "pair_index": index.has_pair_index(),
               "kmer_k": index.kmer_k(), "steps": args.steps, "runs": args.runs, "mean_length": mean_len,
               "seeds": nseeds,
               "match_stats": med(lambda: stats(0), args.steps),
               "match_stats_seed_filter": med(lambda: stats(args.min_seed_len), args.steps),
               "emulation_suffix_match_on_prefix_copies": med(emulation, max(args.steps // 2, 1)),
               "count_same_batch": med(count_call, args.steps)}
        rec["slots_per_s"] = round(total / (rec["match_stats"]["median_ms"] * 1e-3))
        rec["count_times_plen_ms"] = round(rec["count_same_batch"]["median_ms"] * m, 4)
        print(json.dumps(rec), flush=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(rec) + "\n")
    index.close()
