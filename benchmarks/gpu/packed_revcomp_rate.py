"""fmx_count_batch_packed2_rc* (both strands of every pattern in one call) against its emulation on the config-2 DNA
text (fm_index_amd.workload.dna_text_torch, seed 1), the protocol of packed_count_rate.py: one session, two indexes of
the same text -- the default one (pair index + k-mer table) and plain=True -- and three sets of `--npat` patterns of
`--plen` symbols
    substring   substrings of the text        one_changed   one symbol changed        random   uniform over 1..4
The EMULATION is what a caller had to do before: fmx_count_batch_packed2[_dev] on a batch of 2 * npat patterns that
holds every pattern followed by its reverse complement (so its slots are the call's slots).  Making and packing the
complements is NOT timed, which favours the emulation.  Per (index, set):
    resident    fmx_count_batch_packed2_rc_dev on the npat-pattern stream and fmx_count_batch_packed2_dev on the
                2 npat-pattern stream: HIP-event time per call, mean of --steps back-to-back calls, median of --runs runs
    pageable    the host forms from pageable numpy arrays: host clock around --steps back-to-back (synchronous) calls,
                median of --runs runs
    pinned      the same from page-locked arrays, inputs and outputs (torch pin_memory)
Every result of the call is compared with the emulation's before anything is timed.  --out is rewritten with one JSON
line per (index, set); `slower_beyond_spread` lists the legs where the call's median is above the emulation's by more
than the spread (max - min) of the emulation's own runs.
    python benchmarks/gpu/packed_revcomp_rate.py --out profiles/r14/packed_revcomp.jsonl"""
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
ap.add_argument("--out", default="profiles/r14/packed_revcomp.jsonl")
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


def check(rc):
    if rc != 0:
        raise RuntimeError(lib.fmx_last_error().decode())


# ---- the three pattern sets (as packed_count_rate.py makes them) ----
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
off1_h = np.arange(npat + 1, dtype=np.uint64) * np.uint64(m)          # the call's offsets
off2_h = np.arange(2 * npat + 1, dtype=np.uint64) * np.uint64(m)      # the emulation's: 2 npat patterns
off1, off2 = (torch.from_numpy(o.view(np.int64)).to(dev) for o in (off1_h, off2_h))
off1_p, off2_p = (torch.from_numpy(o.view(np.int64)).pin_memory() for o in (off1_h, off2_h))
d_out = [torch.empty(2 * npat, dtype=torch.int64, device=dev) for _ in range(6)]   # emulation s, e, c; call s, e, c
h_out = [np.zeros(2 * npat, dtype=np.uint64) for _ in range(6)]
p_out = [torch.zeros(2 * npat, dtype=torch.int64).pin_memory() for _ in range(6)]


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


os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
open(args.out, "w").close()                           # a run replaces the file: one record per (index, set)
for iname, kw in (("default", {}), ("plain", {"plain": True})):
    index = F.FMIndex.from_device_text(text.data_ptr(), n, 4, device=0, **kw)
    h = index.handle()
    assert index.packed2_rc_supported()
    for sname, pat2d in sets.items():
        # the emulation's batch: pattern k, then its reverse complement (made here, not timed)
        both2d = torch.stack([pat2d, (5 - pat2d.flip(1)).to(torch.uint8)], dim=1).view(2 * npat, m)
        w1_h, _ = F.pack2(flat=pat2d.view(-1).cpu().numpy(), off=off1_h)
        w2_h, _ = F.pack2(flat=both2d.view(-1).cpu().numpy(), off=off2_h)
        del both2d
        w1, w2 = (torch.from_numpy(w.view(np.int64)).to(dev) for w in (w1_h, w2_h))
        w1_p, w2_p = (torch.from_numpy(w.view(np.int64)).pin_memory() for w in (w1_h, w2_h))

        def emul_dev():
            check(lib.fmx_count_batch_packed2_dev(h, P(w2), P(off2), 2 * npat, None, P(d_out[0]), P(d_out[1]),
                                                  P(d_out[2]), sp))

        def rc_dev():
            check(lib.fmx_count_batch_packed2_rc_dev(h, P(w1), P(off1), npat, P(d_out[3]), P(d_out[4]), P(d_out[5]), sp))

        def emul_host():
            check(lib.fmx_count_batch_packed2(h, w2_h.ctypes.data, off2_h.ctypes.data, 2 * npat, None,
                                              h_out[0].ctypes.data, h_out[1].ctypes.data, h_out[2].ctypes.data))

        def rc_host():
            check(lib.fmx_count_batch_packed2_rc(h, w1_h.ctypes.data, off1_h.ctypes.data, npat, h_out[3].ctypes.data,
                                                 h_out[4].ctypes.data, h_out[5].ctypes.data))

        def emul_pinned():
            check(lib.fmx_count_batch_packed2(h, P(w2_p), P(off2_p), 2 * npat, None, P(p_out[0]), P(p_out[1]),
                                              P(p_out[2])))

        def rc_pinned():
            check(lib.fmx_count_batch_packed2_rc(h, P(w1_p), P(off1_p), npat, P(p_out[3]), P(p_out[4]), P(p_out[5])))

        # ---- results first: every form against the resident emulation ----
        emul_dev(); rc_dev(); emul_host(); rc_host(); emul_pinned(); rc_pinned()
        torch.cuda.synchronize()
        assert lib.fmx_stream_status(h) == 0
        want = [d_out[q].cpu().numpy().view(np.uint64) for q in range(3)]
        for q in range(3):
            assert (d_out[3 + q].cpu().numpy().view(np.uint64) == want[q]).all(), (iname, sname, "resident", q)
            assert (h_out[q] == want[q]).all() and (h_out[3 + q] == want[q]).all(), (iname, sname, "pageable", q)
            assert (p_out[q].numpy().view(np.uint64) == want[q]).all(), (iname, sname, "pinned emulation", q)
            assert (p_out[3 + q].numpy().view(np.uint64) == want[q]).all(), (iname, sname, "pinned call", q)
        t = {"resident_emul": med(emul_dev, event_ms), "resident_rc": med(rc_dev, event_ms),
             "pageable_emul": med(emul_host, host_ms), "pageable_rc": med(rc_host, host_ms),
             "pinned_emul": med(emul_pinned, host_ms), "pinned_rc": med(rc_pinned, host_ms)}
        legs = ("resident", "pageable", "pinned")
        rec = {"index": iname, "set": sname, "log2n": args.log2n, "npat": npat, "plen": m,
               "pair_index": index.has_pair_index(), "kmer_k": index.kmer_k(), "steps": args.steps, "runs": args.runs,
               "matching_forward": int((want[2][0::2] > 0).sum()), "matching_revcomp": int((want[2][1::2] > 0).sum()),
               **t,
               **{"speedup_" + g: round(t[g + "_emul"]["median_ms"] / t[g + "_rc"]["median_ms"], 3) for g in legs},
               "slower_beyond_spread": [g for g in legs if t[g + "_rc"]["median_ms"] - t[g + "_emul"]["median_ms"] >
                                        t[g + "_emul"]["max_ms"] - t[g + "_emul"]["min_ms"]],
               "pattern_chars_per_s_resident_rc": round(2 * npat * m / (t["resident_rc"]["median_ms"] * 1e-3), 0)}
        print(json.dumps(rec), flush=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(rec) + "\n")
        del w1, w2, w1_p, w2_p
    index.close()
