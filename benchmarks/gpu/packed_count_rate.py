"""fmx_count_batch_packed2* against fmx_count_batch* on the config-2 DNA text (fm_index_amd.workload.dna_text_torch,
seed 1), the protocol of suffix_match_rate.py: one session, two indexes of the same text -- the default one (pair index
+ k-mer table) and plain=True -- and three sets of `--npat` patterns of `--plen` symbols
    substring   substrings of the text        one_changed   one symbol changed        random   uniform over 1..4
each as bytes and as the 2-bit packed stream of include/fmx.h (fm_index_amd.pack2).  Per (index, set):
    resident    fmx_count_batch_packed2_dev and fmx_count_batch_dev on the same resident batch: HIP-event time per call,
                mean of --steps back-to-back calls, median of --runs runs
    pageable    fmx_count_batch_packed2 and fmx_count_batch from pageable numpy arrays: host clock around --steps
                back-to-back (synchronous) calls, median of --runs runs
    pinned      the same from page-locked arrays, inputs and outputs (torch pin_memory)
The packed results are compared with the byte results before anything is timed.  --out is rewritten with one JSON line
per (index, set); `byte_in_recorded_range` says whether the resident byte call of the substring set lies inside the
range README.md records for it (0.305-0.348 ms default, 0.62-0.64 ms plain at 2^30 / 2^20 x 32): a session where it does
not is not comparable.
    python benchmarks/gpu/packed_count_rate.py --out profiles/r13/packed_count.jsonl"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.getcwd())
import numpy as np
import torch

import fm_index_amd as F
from fm_index_amd import _lib as L
from fm_index_amd import workload as W

ap = argparse.ArgumentParser()
ap.add_argument("--log2n", type=int, default=30)
ap.add_argument("--npat", type=int, default=1 << 20)
ap.add_argument("--plen", type=int, default=32)
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--out", default="profiles/r13/packed_count.jsonl")
args = ap.parse_args()

dev = torch.device("cuda", 0)
torch.cuda.set_device(0)
lib = L.lib()
n, npat, m = 1 << args.log2n, args.npat, args.plen
text = W.dna_text_torch(n, 1, dev)
stream = torch.cuda.current_stream()
sp = C.c_void_p(stream.cuda_stream)
RANGES = {"default": (0.305, 0.348), "plain": (0.62, 0.64)}


def P(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def check(rc):
    if rc != 0:
        raise RuntimeError(lib.fmx_last_error().decode())


# ---- the three pattern sets (as suffix_match_rate.py makes them) ----
src = W.umod_torch(W.splitmix64_torch(3, 0, npat, dev), n - 1 - m)
sub = text[src[:, None] + torch.arange(m, dtype=torch.int64, device=dev)[None, :]].contiguous()
where = W.umod_torch(W.splitmix64_torch(11, 0, npat, dev), m)
bump = W.umod_torch(W.splitmix64_torch(12, 0, npat, dev), 3) + 1                    # 1..3: always another symbol
changed = sub.clone()
rows = torch.arange(npat, device=dev)
changed[rows, where] = ((changed[rows, where].to(torch.int64) - 1 + bump) % 4 + 1).to(torch.uint8)
rnd = (W.umod_torch(W.splitmix64_torch(13, 0, npat * m, dev), 4) + 1).to(torch.uint8).view(npat, m).contiguous()
sets = {"substring": sub, "one_changed": changed, "random": rnd}
del src, where, bump, rows
off_h = np.arange(npat + 1, dtype=np.uint64) * np.uint64(m)
off = torch.from_numpy(off_h.view(np.int64)).to(dev)
d_out = [torch.empty(npat, dtype=torch.int64, device=dev) for _ in range(6)]       # byte s, e, c; packed s, e, c
h_out = [np.zeros(npat, dtype=np.uint64) for _ in range(6)]
p_out = [torch.zeros(npat, dtype=torch.int64).pin_memory() for _ in range(6)]
off_p = torch.from_numpy(off_h.view(np.int64)).pin_memory()


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(args.steps):
        fn()
    e1.record(stream)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / args.steps


def host_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        fn()                                          # synchronous: returns with the results in the caller's arrays
    return (time.perf_counter() - t0) * 1e3 / args.steps


def med(fn, clock):
    fn()
    torch.cuda.synchronize()
    xs = [clock(fn) for _ in range(args.runs)]
    return {"median_ms": round(statistics.median(xs), 4), "min_ms": round(min(xs), 4), "max_ms": round(max(xs), 4)}


def ratio(byte, packed):
    return round(byte["median_ms"] / packed["median_ms"], 3)


os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
open(args.out, "w").close()                           # a run replaces the file: one record per (index, set)
for iname, kw in (("default", {}), ("plain", {"plain": True})):
    index = F.FMIndex.from_device_text(text.data_ptr(), n, 4, device=0, **kw)
    h = index.handle()
    assert index.packed2_supported()
    for sname, pat2d in sets.items():
        flat = pat2d.view(-1)
        flat_h = flat.cpu().numpy()
        words_h, _ = F.pack2(flat=flat_h, off=off_h)
        words = torch.from_numpy(words_h.view(np.int64)).to(dev)
        flat_p, words_p = torch.from_numpy(flat_h).pin_memory(), torch.from_numpy(words_h.view(np.int64)).pin_memory()

        def byte_dev():
            check(lib.fmx_count_batch_dev(h, P(flat), P(off), npat, None, P(d_out[0]), P(d_out[1]), P(d_out[2]), sp))

        def packed_dev():
            check(lib.fmx_count_batch_packed2_dev(h, P(words), P(off), npat, None, P(d_out[3]), P(d_out[4]),
                                                  P(d_out[5]), sp))

        def byte_host():
            check(lib.fmx_count_batch(h, flat_h.ctypes.data, off_h.ctypes.data, npat, None, h_out[0].ctypes.data,
                                      h_out[1].ctypes.data, h_out[2].ctypes.data))

        def packed_host():
            check(lib.fmx_count_batch_packed2(h, words_h.ctypes.data, off_h.ctypes.data, npat, None,
                                              h_out[3].ctypes.data, h_out[4].ctypes.data, h_out[5].ctypes.data))

        def byte_pinned():
            check(lib.fmx_count_batch(h, P(flat_p), P(off_p), npat, None, P(p_out[0]), P(p_out[1]), P(p_out[2])))

        def packed_pinned():
            check(lib.fmx_count_batch_packed2(h, P(words_p), P(off_p), npat, None, P(p_out[3]), P(p_out[4]),
                                              P(p_out[5])))

        # ---- results first: every packed form against the resident byte call ----
        byte_dev(); packed_dev(); byte_host(); packed_host(); byte_pinned(); packed_pinned()
        torch.cuda.synchronize()
        assert lib.fmx_stream_status(h) == 0
        want = [d_out[q].cpu().numpy().view(np.uint64) for q in range(3)]
        for q in range(3):
            assert (d_out[3 + q].cpu().numpy().view(np.uint64) == want[q]).all(), (iname, sname, "resident", q)
            assert (h_out[q] == want[q]).all() and (h_out[3 + q] == want[q]).all(), (iname, sname, "pageable", q)
            assert (p_out[q].numpy().view(np.uint64) == want[q]).all(), (iname, sname, "pinned bytes", q)
            assert (p_out[3 + q].numpy().view(np.uint64) == want[q]).all(), (iname, sname, "pinned packed", q)
        t = {"resident_byte": med(byte_dev, event_ms), "resident_packed": med(packed_dev, event_ms),
             "pageable_byte": med(byte_host, host_ms), "pageable_packed": med(packed_host, host_ms),
             "pinned_byte": med(byte_pinned, host_ms), "pinned_packed": med(packed_pinned, host_ms)}
        lo, hi = RANGES[iname]
        rec = {"index": iname, "set": sname, "log2n": args.log2n, "npat": npat, "plen": m,
               "pair_index": index.has_pair_index(), "kmer_k": index.kmer_k(), "steps": args.steps, "runs": args.runs,
               "matching_patterns": int((want[2] > 0).sum()), **t,
               "speedup_resident": ratio(t["resident_byte"], t["resident_packed"]),
               "speedup_pageable": ratio(t["pageable_byte"], t["pageable_packed"]),
               "speedup_pinned": ratio(t["pinned_byte"], t["pinned_packed"]),
               "pattern_chars_per_s_resident_packed": round(npat * m / (t["resident_packed"]["median_ms"] * 1e-3), 0),
               "byte_in_recorded_range": (lo <= t["resident_byte"]["median_ms"] <= hi) if sname == "substring" and
               (args.log2n, npat, m) == (30, 1 << 20, 32) else None}
        print(json.dumps(rec), flush=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(rec) + "\n")
        del words, flat_p, words_p
    index.close()
