"""fmx_count_windows_packed2*_dev against its emulation, fmx_count_batch_packed2*_dev on the EXPANDED batch (every
window written out as a pattern of its own), on the config-2 DNA text (fm_index_amd.workload.dna_text_torch, seed 1).
One session, two indexes of the same text -- the default one (pair index + k-mer table) and plain=True -- and per index
    set      substring: one substring of the text (every window occurs)      random: uniform over 1..4
    k        32 and 21, on one resident sequence of --windows + 31 symbols (so --windows windows at k = 32)
    strands  1 (fmx_count_windows_packed2_dev / fmx_count_batch_packed2_dev) and 2 (the _rc forms)
Both legs are resident; the expansion is made and the results are compared before anything is timed.  HIP-event time
per call, mean of --steps back-to-back calls; --runs runs per leg, the legs ALTERNATING; median, min and max per leg.
`expanded_bytes` is what the emulation needs in device memory for its words and offsets, `sequence_bytes` what the
window call needs.  --out is rewritten with one JSON line per (index, set, k, strands).
    python benchmarks/gpu/window_count_rate.py --out profiles/r18/window_count.jsonl"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.getcwd())
import numpy as np
import torch

import fm_index_amd as F
from fm_index_amd import _lib as L
from fm_index_amd import workload as W

ap = argparse.ArgumentParser()
ap.add_argument("--log2n", type=int, default=30)
ap.add_argument("--windows", type=int, default=1 << 20)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--out", default="profiles/r18/window_count.jsonl")
args = ap.parse_args()

dev = torch.device("cuda", 0)
torch.cuda.set_device(0)
lib = L.lib()
n, m = 1 << args.log2n, args.windows + 31
text = W.dna_text_torch(n, 1, dev)
stream = torch.cuda.current_stream()
sp = C.c_void_p(stream.cuda_stream)


def P(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def check(rc):
    if rc != 0:
        raise RuntimeError(lib.fmx_last_error().decode())


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to(dev)


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(args.steps):
        fn()
    e1.record(stream)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / args.steps


def stats(xs):
    return {"median_ms": round(statistics.median(xs), 4), "min_ms": round(min(xs), 4), "max_ms": round(max(xs), 4)}


start = int(W.splitmix64_np(3, 0, 1)[0] % np.uint64(n - 1 - m))
sets = {"substring": text[start:start + m].cpu().numpy(),
        "random": (W.splitmix64_np(13, 0, m) % np.uint64(4)).astype(np.uint8) + 1}
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
open(args.out, "w").close()                           # a run replaces the file
for iname, kw in (("default", {}), ("plain", {"plain": True})):
    index = F.FMIndex.from_device_text(text.data_ptr(), n, 4, device=0, **kw)
    h = index.handle()
    assert index.packed2_rc_supported()
    for sname, seq in sets.items():
        seq_off_h = np.array([0, m], dtype=np.uint64)
        seq_words, seq_off = to_dev(F.pack2(flat=seq, off=seq_off_h)[0]), to_dev(seq_off_h)
        for k in (32, 21):
            nwin = m - k + 1
            # ---- the emulation's input: every window as a pattern of its own, made before anything is timed ----
            exp = np.lib.stride_tricks.sliding_window_view(seq, k).reshape(-1)
            exp_off_h = np.arange(nwin + 1, dtype=np.uint64) * np.uint64(k)
            exp_words_h = F.pack2(flat=exp, off=exp_off_h)[0]
            exp_words, exp_off = to_dev(exp_words_h), to_dev(exp_off_h)
            for strands in (1, 2):
                w_out = [torch.empty(strands * m, dtype=torch.int64, device=dev) for _ in range(3)]
                y_out = [torch.empty(strands * nwin, dtype=torch.int64, device=dev) for _ in range(3)]

                def windows():
                    f = lib.fmx_count_windows_packed2_rc_dev if strands == 2 else lib.fmx_count_windows_packed2_dev
                    check(f(h, P(seq_words), P(seq_off), 1, m, k, P(w_out[0]), P(w_out[1]), P(w_out[2]), sp))

                def yardstick():
                    if strands == 2:
                        check(lib.fmx_count_batch_packed2_rc_dev(h, P(exp_words), P(exp_off), nwin, P(y_out[0]),
                                                                 P(y_out[1]), P(y_out[2]), sp))
                    else:
                        check(lib.fmx_count_batch_packed2_dev(h, P(exp_words), P(exp_off), nwin, None, P(y_out[0]),
                                                              P(y_out[1]), P(y_out[2]), sp))

                windows(); yardstick()                # results first (and the warm-up of both legs)
                torch.cuda.synchronize()
                assert lib.fmx_stream_status(h) == 0
                for a, b in zip(w_out, y_out):
                    assert torch.equal(a[:strands * nwin], b) and not a[strands * nwin:].any(), (iname, sname, k, strands)
                tw, ty = [], []
                for _ in range(args.runs):            # the legs alternate
                    tw.append(event_ms(windows))
                    ty.append(event_ms(yardstick))
                tw, ty = stats(tw), stats(ty)
                rec = {"index": iname, "set": sname, "log2n": args.log2n, "k": k, "strands": strands, "windows": nwin,
                       "pair_index": index.has_pair_index(), "kmer_k": index.kmer_k(), "steps": args.steps,
                       "runs": args.runs, "windows_with_a_match": int((y_out[2] > 0).sum()),
                       "window_call": tw, "expanded_batch": ty,
                       "speedup": round(ty["median_ms"] / tw["median_ms"], 3),
                       "windows_per_s": round(strands * nwin / (tw["median_ms"] * 1e-3), 0),
                       "sequence_bytes": int(seq_words.numel() * 8 + 16),
                       "expanded_bytes": int(exp_words_h.nbytes + exp_off_h.nbytes)}
                print(json.dumps(rec), flush=True)
                with open(args.out, "a") as f:
                    f.write(json.dumps(rec) + "\n")
            del exp_words, exp_off
    index.close()
