"""fmx_suffix_match_batch_dev against fmx_count_batch_dev and against the per-symbol emulation it replaces, on the
config-2 DNA text (fm_index_amd.workload.dna_text_torch, seed 1; patterns as benchmarks/legs/common.py makes them).

Two indexes of the same text -- the default one (pair index + k-mer table from 2^24 symbols) and plain=True -- and three
sets of `--npat` patterns of `--plen` symbols, all resident on the device:
    substring   substrings of the text (every pattern matches in full, L = plen)
    one_changed substrings with one symbol changed (to another symbol of 1..4) at a uniform position
    random      uniform random patterns over 1..4
For each: the new call, fmx_count_batch_dev on the same batch, and the emulation -- `plen` rounds of fmx_count_batch_dev
with s0e0, one symbol per round, DECIDED ON THE DEVICE (torch element-wise kernels between the rounds keep the last
interval of >= min_count rows and the matched length into buffers allocated once; no host synchronisation, all rounds
are always launched).  Times are HIP-event times per call (mean of --steps back-to-back calls), median of --runs runs;
--out is rewritten with one JSON line per (index, set).  The emulation's result is compared with the new call's before anything is timed.
    python benchmarks/gpu/suffix_match_rate.py --out profiles/r09/suffix_match.jsonl"""
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
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--out", default="profiles/r09/suffix_match.jsonl")
args = ap.parse_args()

dev = torch.device("cuda", 0)
torch.cuda.set_device(0)
lib = L.lib()
n, npat, m, mc = 1 << args.log2n, args.npat, args.plen, max(args.min_count, 1)
text = W.dna_text_torch(n, 1, dev)
stream = torch.cuda.current_stream()
sp = C.c_void_p(stream.cuda_stream)


def P(t):
    return None if t is None else C.c_void_p(t.data_ptr())


# ---- the three pattern sets ----
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
off1 = torch.arange(npat + 1, dtype=torch.int64, device=dev).contiguous()
d_s, d_e, d_c, d_l = (torch.empty(npat, dtype=torch.int64, device=dev) for _ in range(4))
e_s, e_e, width, tmp, length = (torch.empty(npat, dtype=torch.int64, device=dev) for _ in range(5))   # the emulation's
se = torch.zeros(npat, 2, dtype=torch.int64, device=dev)
alive, passed = (torch.empty(npat, dtype=torch.bool, device=dev) for _ in range(2))


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
        cols = pat2d.t().contiguous()                 # cols[j] = symbol j of every pattern: round r reads cols[m - 1 - r]

        def new_call():
            check(lib.fmx_suffix_match_batch_dev(h, P(flat), P(off), npat, None, mc, P(d_s), P(d_e), P(d_c), P(d_l), sp))

        def count_call():
            check(lib.fmx_count_batch_dev(h, P(flat), P(off), npat, None, P(d_s), P(d_e), P(d_c), sp))

        def emulation():           # (every buffer allocated once, above: no allocation inside the timed calls)
            se.zero_()
            se[:, 1].fill_(n)
            length.zero_()
            alive.fill_(True)
            for r in range(m):
                check(lib.fmx_count_batch_dev(h, P(cols[m - 1 - r]), P(off1), npat, P(se), P(e_s), P(e_e), None, sp))
                torch.sub(e_e, e_s, out=width)
                torch.ge(width, mc, out=passed)
                alive.logical_and_(passed)
                torch.where(alive, e_s, se[:, 0], out=tmp)
                se[:, 0].copy_(tmp)
                torch.where(alive, e_e, se[:, 1], out=tmp)
                se[:, 1].copy_(tmp)
                length.add_(alive)
            return se, length

        new_call()
        se, length = emulation()
        torch.cuda.synchronize()
        assert lib.fmx_stream_status(h) == 0
        assert bool((se[:, 0] == d_s).all()) and bool((se[:, 1] == d_e).all()) and bool((length == d_l).all())
        rec = {"index": iname, "set": sname, "log2n": args.log2n, "npat": npat, "plen": m, "min_count": mc,
               "pair_index": index.has_pair_index(), "kmer_k": index.kmer_k(), "steps": args.steps, "runs": args.runs,
               "mean_matched_length": round(float(d_l.double().mean().item()), 3),
               # patterns whose k-mer table entry was not taken (every pattern here asks the table): those with L < k
               "table_misses": int((d_l < index.kmer_k()).sum().item()) if index.kmer_k() else None,
               "suffix_match": med(new_call, args.steps), "count": med(count_call, args.steps),
               "emulation_device_decided": med(emulation, max(args.steps // 5, 1))}
        print(json.dumps(rec), flush=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(rec) + "\n")
    index.close()
