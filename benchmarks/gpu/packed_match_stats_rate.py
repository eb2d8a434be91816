"""fmx_match_stats_batch_packed2* and fmx_match_stats_batch_packed2_rc* against the byte call on the config-2 DNA text
(fm_index_amd.workload.dna_text_torch, seed 1), the protocol of match_stats_rate.py and packed_revcomp_rate.py: one
session, two indexes of the same text -- the default one (pair index + k-mer table) and plain=True -- and three sets of
`--npat` patterns of `--plen` symbols
    substring   substrings of the text        one_changed   one symbol changed        random   uniform over 1..4
The YARDSTICK is the byte call of the same session, never the code under test:
    single strand   fmx_match_stats_batch[_dev] on the byte form of the same batch
    both strands    the same on the 2 npat virtual batch P_0, R_0, P_1, R_1, ... with host-made reverse complements;
                    making them is NOT timed, which favours the yardstick
Per (index, set, min_seed_len in --seed-lens):
    resident    the dev forms on resident patterns: HIP-event time per call, mean of --steps back-to-back calls, median
                of --runs runs
and per (index, set in --host-sets), min_seed_len 0:
    pageable    the host forms from pageable numpy arrays: host clock around --steps back-to-back (synchronous) calls
    pinned      the same from page-locked arrays, inputs and outputs (torch pin_memory)
Every array of every form is compared with the yardstick's before anything is timed.  --out is rewritten with one JSON
line per (index, set, min_seed_len); `slower_beyond_spread` lists the legs whose median is above the yardstick's by more
than the spread (max - min) of the yardstick's own runs.
    python benchmarks/gpu/packed_match_stats_rate.py --out profiles/r15/packed_match_stats.jsonl"""
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
ap.add_argument("--seed-lens", default="0,19")
ap.add_argument("--host-sets", default="one_changed")
ap.add_argument("--out", default="profiles/r15/packed_match_stats.jsonl")
args = ap.parse_args()

dev = torch.device("cuda", 0)
torch.cuda.set_device(0)
lib = L.lib()
n, npat, m = 1 << args.log2n, args.npat, args.plen
total = npat * m
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
off1_h = np.arange(npat + 1, dtype=np.uint64) * np.uint64(m)          # the batch, and the packed calls' offsets
off2_h = np.arange(2 * npat + 1, dtype=np.uint64) * np.uint64(m)      # the virtual batch of both strands
off1, off2 = (torch.from_numpy(o.view(np.int64)).to(dev) for o in (off1_h, off2_h))
off1_p, off2_p = (torch.from_numpy(o.view(np.int64)).pin_memory() for o in (off1_h, off2_h))
d_out = [torch.empty(2 * total, dtype=torch.int64, device=dev) for _ in range(6)]   # yardstick s, e, len; call s, e, len
host_legs = bool(args.host_sets)
h_out = [np.zeros(2 * total, dtype=np.uint64) for _ in range(3)] if host_legs else None
p_out = [torch.zeros(2 * total, dtype=torch.int64).pin_memory() for _ in range(3)] if host_legs else None


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
open(args.out, "w").close()                           # a run replaces the file
for iname, kw in (("default", {}), ("plain", {"plain": True})):
    index = F.FMIndex.from_device_text(text.data_ptr(), n, 4, device=0, **kw)
    h = index.handle()
    assert index.packed2_rc_supported()
    for sname, pat2d in sets.items():
        # the yardstick's batches: the bytes, and every pattern followed by its reverse complement (not timed)
        b1 = pat2d.view(-1)
        b2 = torch.stack([pat2d, (5 - pat2d.flip(1)).to(torch.uint8)], dim=1).view(-1).contiguous()
        b1_h, b2_h = b1.cpu().numpy(), b2.cpu().numpy()
        w_h, _ = F.pack2(flat=b1_h, off=off1_h)
        w = torch.from_numpy(w_h.view(np.int64)).to(dev)
        for msl in [int(x) for x in args.seed_lens.split(",")]:
            # (name, strands): the yardstick and the call under test, resident
            def byte_dev(strands):
                check(lib.fmx_match_stats_batch_dev(h, P(b2 if strands == 2 else b1), P(off2 if strands == 2 else off1),
                                                    strands * npat, strands * total, 1, 0, msl, P(d_out[0]),
                                                    P(d_out[1]), P(d_out[2]), sp))

            def packed_dev(strands):
                f = lib.fmx_match_stats_batch_packed2_rc_dev if strands == 2 else lib.fmx_match_stats_batch_packed2_dev
                check(f(h, P(w), P(off1), npat, total, 1, 0, msl, P(d_out[3]), P(d_out[4]), P(d_out[5]), sp))

            def byte_host(strands, pin):
                o = p_out if pin else h_out
                a = (b2_p, off2_p) if pin and strands == 2 else (b1_p, off1_p) if pin else \
                    (b2_h, off2_h) if strands == 2 else (b1_h, off1_h)
                check(lib.fmx_match_stats_batch(h, P(a[0]) if pin else a[0].ctypes.data,
                                                P(a[1]) if pin else a[1].ctypes.data, strands * npat, 1, 0, msl,
                                                *[P(x) if pin else x.ctypes.data for x in o]))

            def packed_host(strands, pin):
                f = lib.fmx_match_stats_batch_packed2_rc if strands == 2 else lib.fmx_match_stats_batch_packed2
                o = p_out if pin else h_out
                check(f(h, P(w_p) if pin else w_h.ctypes.data, P(off1_p) if pin else off1_h.ctypes.data, npat, 1, 0, msl,
                        *[P(x) if pin else x.ctypes.data for x in o]))

            host = host_legs and msl == 0 and sname in args.host_sets.split(",")
            if host:
                b1_p, b2_p, w_p = (torch.from_numpy(x.view(np.int64) if x.dtype == np.uint64 else x).pin_memory()
                                   for x in (b1_h, b2_h, w_h))
            rec = {"index": iname, "set": sname, "min_seed_len": msl, "log2n": args.log2n, "npat": npat, "plen": m,
                   "pair_index": index.has_pair_index(), "kmer_k": index.kmer_k(), "steps": args.steps,
                   "runs": args.runs, "slower_beyond_spread": []}
            for strands, tag in ((1, "single"), (2, "both")):
                # ---- results first: every form against the resident yardstick ----
                ns = strands * total
                byte_dev(strands); packed_dev(strands)
                torch.cuda.synchronize()
                assert lib.fmx_stream_status(h) == 0
                want = [d_out[q][:ns].cpu().numpy().view(np.uint64) for q in range(3)]
                for q in range(3):
                    assert (d_out[3 + q][:ns].cpu().numpy().view(np.uint64) == want[q]).all(), (iname, sname, tag, q)
                forms = [("resident", lambda: byte_dev(strands), lambda: packed_dev(strands), event_ms)]
                if host:
                    for pin, leg in ((False, "pageable"), (True, "pinned")):
                        for fn in (byte_host, packed_host):
                            fn(strands, pin)
                            for q in range(3):
                                got = p_out[q].numpy().view(np.uint64) if pin else h_out[q]
                                assert (got[:ns] == want[q]).all(), (iname, sname, tag, leg, fn.__name__, q)
                        forms.append((leg, lambda pin=pin: byte_host(strands, pin),
                                      lambda pin=pin: packed_host(strands, pin), host_ms))
                for leg, yard, call, clock in forms:
                    ty, tc = med(yard, clock), med(call, clock)
                    rec["%s_%s_byte" % (leg, tag)], rec["%s_%s_packed" % (leg, tag)] = ty, tc
                    rec["speedup_%s_%s" % (leg, tag)] = round(ty["median_ms"] / tc["median_ms"], 3)
                    if tc["median_ms"] - ty["median_ms"] > ty["max_ms"] - ty["min_ms"]:
                        rec["slower_beyond_spread"].append("%s_%s" % (leg, tag))
                rec["slots_%s" % tag] = ns
                rec["mean_len_%s" % tag] = round(float(want[2].mean()), 3)
                rec["seeds_%s" % tag] = int((want[1] > want[0]).sum())
            print(json.dumps(rec), flush=True)
            with open(args.out, "a") as f:
                f.write(json.dumps(rec) + "\n")
        del w, b2
    index.close()
