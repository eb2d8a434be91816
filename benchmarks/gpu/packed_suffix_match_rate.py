"""fmx_suffix_match_batch_packed2* against fmx_suffix_match_batch* on the config-2 DNA text
(fm_index_amd.workload.dna_text_torch, seed 1), the protocol of suffix_match_rate.py and packed_count_rate.py: one
session, two indexes of the same text -- the default one (pair index + k-mer table) and plain=True -- and three sets of
`--npat` patterns of `--plen` symbols
    substring   substrings of the text        one_changed   one symbol changed        random   uniform over 1..4
each as bytes and as the 2-bit packed stream of include/fmx.h (fm_index_amd.pack2), min_count 1.  Per (index, set):
    resident    one strand: fmx_suffix_match_batch_packed2_dev against fmx_suffix_match_batch_dev on the same batch;
                both strands: fmx_suffix_match_batch_packed2_rc_dev against fmx_suffix_match_batch_dev on the virtual
                batch P_0, R_0, P_1, R_1, ... of 2 npat patterns whose reverse complements are made beforehand (not
                timed); the emulation a holder of packed reads has today, fmx_match_stats_batch_packed2_dev with every
                slot but a pattern's last thrown away.  HIP-event time per call, mean of --steps back-to-back calls,
                median of --runs runs in which the legs alternate; min and max of the runs are the session's spread
    pageable    fmx_suffix_match_batch_packed2[_rc] and fmx_suffix_match_batch from pageable numpy arrays: host clock
                around --steps back-to-back (synchronous) calls, median of --runs runs
    pinned      the same from page-locked arrays, inputs and outputs (torch pin_memory)
Every packed result is compared with the byte result before anything is timed.  --out is rewritten with one JSON line
per (index, set).
    python benchmarks/gpu/packed_suffix_match_rate.py --out profiles/r17/packed_suffix_match.jsonl"""
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
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--out", default="profiles/r17/packed_suffix_match.jsonl")
args = ap.parse_args()

dev = torch.device("cuda", 0)
torch.cuda.set_device(0)
lib = L.lib()
n, npat, m = 1 << args.log2n, args.npat, args.plen
text = W.dna_text_torch(n, 1, dev)
stream = torch.cuda.current_stream()
sp = C.c_void_p(stream.cuda_stream)


def P(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def H(a):
    return a.ctypes.data


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
voff_h = np.arange(2 * npat + 1, dtype=np.uint64) * np.uint64(m)
off = torch.from_numpy(off_h.view(np.int64)).to(dev)
voff = torch.from_numpy(voff_h.view(np.int64)).to(dev)
d_byte = [torch.empty(2 * npat, dtype=torch.int64, device=dev) for _ in range(4)]   # s, e, count, L
d_pack = [torch.empty(2 * npat, dtype=torch.int64, device=dev) for _ in range(4)]
d_ms = [torch.empty(npat * m, dtype=torch.int64, device=dev) for _ in range(3)]     # the emulation's slots
h_byte = [np.zeros(npat, dtype=np.uint64) for _ in range(4)]
h_pack = [np.zeros(2 * npat, dtype=np.uint64) for _ in range(4)]
p_byte = [torch.zeros(npat, dtype=torch.int64).pin_memory() for _ in range(4)]
p_pack = [torch.zeros(2 * npat, dtype=torch.int64).pin_memory() for _ in range(4)]
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


def med(legs, clock):
    """{name: fn} -> {name: median / min / max}; the legs ALTERNATE inside a run, so drift hits all of them alike"""
    for fn in legs.values():
        fn()
    torch.cuda.synchronize()
    xs = {name: [] for name in legs}
    for _ in range(args.runs):
        for name, fn in legs.items():
            xs[name].append(clock(fn))
    return {name: {"median_ms": round(statistics.median(x), 4), "min_ms": round(min(x), 4), "max_ms": round(max(x), 4)}
            for name, x in xs.items()}


def u64(t, k=None):
    return (t.cpu().numpy() if isinstance(t, torch.Tensor) else t).view(np.uint64)[:k]


os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
open(args.out, "w").close()                           # a run replaces the file: one record per (index, set)
for iname, kw in (("default", {}), ("plain", {"plain": True})):
    index = F.FMIndex.from_device_text(text.data_ptr(), n, 4, device=0, **kw)
    h = index.handle()
    assert index.packed2_rc_supported()
    for sname, pat2d in sets.items():
        flat = pat2d.view(-1)
        vflat = torch.stack([pat2d, 5 - pat2d.flip(1)], dim=1).contiguous().view(-1)   # P_0, R_0, P_1, R_1, ...
        flat_h = flat.cpu().numpy()
        words_h, _ = F.pack2(flat=flat_h, off=off_h)
        words = torch.from_numpy(words_h.view(np.int64)).to(dev)
        flat_p, words_p = torch.from_numpy(flat_h).pin_memory(), torch.from_numpy(words_h.view(np.int64)).pin_memory()

        def byte_dev():
            check(lib.fmx_suffix_match_batch_dev(h, P(flat), P(off), npat, None, 1, *map(P, d_byte), sp))

        def packed_dev():
            check(lib.fmx_suffix_match_batch_packed2_dev(h, P(words), P(off), npat, None, 1, *map(P, d_pack), sp))

        def byte_dev_both():
            check(lib.fmx_suffix_match_batch_dev(h, P(vflat), P(voff), 2 * npat, None, 1, *map(P, d_byte), sp))

        def packed_dev_both():
            check(lib.fmx_suffix_match_batch_packed2_rc_dev(h, P(words), P(off), npat, 1, *map(P, d_pack), sp))

        def mstats_dev():
            check(lib.fmx_match_stats_batch_packed2_dev(h, P(words), P(off), npat, npat * m, 1, 0, 0, P(d_ms[0]),
                                                        P(d_ms[1]), P(d_ms[2]), sp))

        def byte_host():
            check(lib.fmx_suffix_match_batch(h, H(flat_h), H(off_h), npat, None, 1, *map(H, h_byte)))

        def packed_host():
            check(lib.fmx_suffix_match_batch_packed2(h, H(words_h), H(off_h), npat, None, 1, *map(H, h_pack)))

        def packed_host_both():
            check(lib.fmx_suffix_match_batch_packed2_rc(h, H(words_h), H(off_h), npat, 1, *map(H, h_pack)))

        def byte_pinned():
            check(lib.fmx_suffix_match_batch(h, P(flat_p), P(off_p), npat, None, 1, *map(P, p_byte)))

        def packed_pinned():
            check(lib.fmx_suffix_match_batch_packed2(h, P(words_p), P(off_p), npat, None, 1, *map(P, p_pack)))

        def packed_pinned_both():
            check(lib.fmx_suffix_match_batch_packed2_rc(h, P(words_p), P(off_p), npat, 1, *map(P, p_pack)))

        # ---- results first: every packed form against the resident byte call on the same strand(s) ----
        def same(got, want, k, what):
            torch.cuda.synchronize()
            assert lib.fmx_stream_status(h) == 0
            for q in range(4):
                assert (u64(got[q], k) == want[q]).all(), (iname, sname, what, q)

        byte_dev_both()
        want2 = [u64(d_byte[q], 2 * npat).copy() for q in range(4)]
        want1 = [w[0::2] for w in want2]
        for fn, got, want, what in ((byte_dev, d_byte, want1, "byte"), (packed_dev, d_pack, want1, "resident"),
                                    (packed_dev_both, d_pack, want2, "resident both"),
                                    (byte_host, h_byte, want1, "pageable byte"), (packed_host, h_pack, want1, "pageable"),
                                    (packed_host_both, h_pack, want2, "pageable both"),
                                    (byte_pinned, p_byte, want1, "pinned byte"), (packed_pinned, p_pack, want1, "pinned"),
                                    (packed_pinned_both, p_pack, want2, "pinned both")):
            fn()
            same(got, want, len(want[0]), what)
        t = med({"resident_byte": byte_dev, "resident_packed": packed_dev, "resident_byte_both": byte_dev_both,
                 "resident_packed_both": packed_dev_both, "resident_match_stats_packed": mstats_dev}, event_ms)
        t.update(med({"pageable_byte": byte_host, "pageable_packed": packed_host,
                      "pageable_packed_both": packed_host_both, "pinned_byte": byte_pinned,
                      "pinned_packed": packed_pinned, "pinned_packed_both": packed_pinned_both}, host_ms))
        r = lambda a, b: round(t[a]["median_ms"] / t[b]["median_ms"], 3)
        rec = {"index": iname, "set": sname, "log2n": args.log2n, "npat": npat, "plen": m, "min_count": 1,
               "pair_index": index.has_pair_index(), "kmer_k": index.kmer_k(), "steps": args.steps, "runs": args.runs,
               "mean_len": round(float(want1[3].mean()), 2), "mean_len_revcomp": round(float(want2[3][1::2].mean()), 2),
               **t, "speedup_resident": r("resident_byte", "resident_packed"),
               "speedup_resident_both": r("resident_byte_both", "resident_packed_both"),
               "speedup_over_match_stats": r("resident_match_stats_packed", "resident_packed"),
               "speedup_pageable": r("pageable_byte", "pageable_packed"),
               "speedup_pinned": r("pinned_byte", "pinned_packed")}
        print(json.dumps(rec), flush=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(rec) + "\n")
        del words, flat_p, words_p, vflat
    index.close()
