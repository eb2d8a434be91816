"""Pattern admission -- what a kernel does before a pattern's first step -- over every kernel shape the dispatch can
select: the same three bad batches through fmx_count_batch_dev, fmx_suffix_match_batch_dev,
fmx_mismatch_count_batch_dev (K = 1) and fmx_match_stats_batch_dev, each where the engine has the call.

    backwards  one pattern has off[k+1] < off[k]
    slice      the batch is a slice (off[0] > 0) and one entry lies below off[0]: the pattern that ends there goes
               backwards and the one that begins there starts below the slice, so both are refused
    start      one start pair has s > len()

Every call must report FMX_ERR_ARG through fmx_stream_status, leave zeros in the outputs of a refused pattern and the
oracle's values in the others (Search::search on the oracle's lf_map2, suffix_match_expect, mismatch_expect and
match_stats_expect, on the patterns the offsets really describe)."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import fm_index_amd as F
from fm_index_amd import _lib as L
from oracle import fm_oracle as O
from match_stats_expect import expect_match_stats
from mismatch_expect import expect_mismatch
from suffix_match_expect import expect_suffix_match
from test_gpu_suffix_match import dna, pieces_text, run_text, sym_text

pytestmark = pytest.mark.gpu

N = 4096
LENS = [6, 8, 4, 4, 12, 5]             # six patterns of 4 .. 12 symbols
LEAD = 8                               # symbols in front of the slice (the whole cut fits between two piece ends)
FILL = 0xDEAD
VARIANTS = ("backwards", "slice", "start")


def _dna(**kw):
    return lambda wide: (F.FMIndexWithLocate(F.Text.with_max_character(TEXTS["dna"], 4), 2, force_wide=wide, **kw),
                         "dna", 4, "fm")


def _rlfm(text, maxc):
    return lambda wide: (F.RLFMIndexWithLocate(F.Text.with_max_character(TEXTS[text], maxc), 2, force_wide=wide),
                         text, maxc, "rlfm")


TEXTS = {"dna": dna(N, 1201), "bytes": sym_text(N, 1202, 200), "u16": sym_text(N, 1203, 1000, np.uint16),
         "pieces": pieces_text(N, 1204), "runs": run_text(N, 1205), "random": sym_text(N, 1206, 200)}
# name -> wide -> (index, text, max_character, oracle kind)
SHAPES = {
    "dna-plain": _dna(plain=True),
    "dna-kmer": _dna(kmer_table=True),
    "dna-pair": _dna(pair_index=True),
    "dna-both": _dna(pair_index=True, kmer_table=True),
    "bytes-two-levels": lambda wide: (F.FMIndexWithLocate(F.Text.with_max_character(TEXTS["bytes"], 200), 2,
                                                          force_wide=wide), "bytes", 200, "fm"),
    "u16": lambda wide: (F.FMIndexWithLocate(F.Text.with_max_character(TEXTS["u16"], 1000), 2, force_wide=wide),
                         "u16", 1000, "fm"),
    "multi-pieces": lambda wide: (F.FMIndexMultiPiecesWithLocate(F.Text.with_max_character(TEXTS["pieces"], 200), 2,
                                                                 force_wide=wide), "pieces", 200, "multi"),
    "rlfm-stored-positions": _rlfm("runs", 5),
    "rlfm-select-blocks": _rlfm("random", 200),
}
# the shapes whose group-per-pattern twins only the measurement build's switches reach
FORCED = ("rlfm-stored-positions", "rlfm-select-blocks", "bytes-two-levels", "multi-pieces")


@functools.lru_cache(maxsize=None)
def oracle(text, maxc, kind):
    return O.OracleIndex(TEXTS[text], maxc, kind=kind) if kind != "fm" else O.OracleIndex(TEXTS[text], maxc)


def patterns(t):
    """LEAD filler symbols and the six patterns behind them, all cut from the text where it holds no 0; the third
    symbol of pattern 4 is changed so that one match ends early"""
    need = LEAD + sum(LENS)
    a = next(a for a in range(100, len(t) - need) if t[a:a + need].min() > 0)
    flat = t[a:a + need].copy()
    for q in (sum(LENS[:4]) + 2, LEAD + sum(LENS[:4]) + 2):          # pattern 4 of a batch from 0 / of the slice
        flat[q] = 1 if flat[q] != 1 else 2
    return np.concatenate([flat, np.zeros(1, dtype=t.dtype)])


def bad_batch(variant, n):
    """(off, s0e0 or None, refused patterns)"""
    off = (LEAD * (variant == "slice") + np.concatenate([[0], np.cumsum(LENS)])).astype(np.uint64)
    if variant == "backwards":                       # pattern 2 ends before it begins; pattern 3 grows to 10 symbols
        off[3] = off[2] - np.uint64(2)
        return off, None, {2}
    if variant == "slice":                           # entry 3 below off[0]: patterns 2 and 3
        off[3] = LEAD - 6
        return off, None, {2, 3}
    se = np.tile(np.array([0, n], dtype=np.uint64), len(LENS))
    se[2 * 4] = n + 1                                # pattern 4: s > len()
    return off, se, {4}


def admitted(flat, off, se, refused, n):
    """the batch the offsets really describe, packed from 0: a refused pattern is empty and starts from (0, len)"""
    pats = [flat[:0] if k in refused else flat[int(off[k]):int(off[k + 1])] for k in range(len(off) - 1)]
    off2 = np.concatenate([[0], np.cumsum([len(p) for p in pats])]).astype(np.uint64)
    flat2 = np.concatenate(pats + [np.zeros(1, dtype=flat.dtype)])
    se2 = None
    if se is not None:
        se2 = se.copy()
        for k in refused:
            se2[2 * k:2 * k + 2] = (0, n)
    return flat2, off2, se2


def expect_count(oi, flat, off, se):
    """Search::search of the reference on the oracle's lf_map2: (s, e, count) of every pattern"""
    npat = len(off) - 1
    s, e = np.zeros(npat, dtype=np.uint64), np.full(npat, len(oi), dtype=np.uint64)
    if se is not None:
        s, e = se[0::2].copy(), se[1::2].copy()
    for k in range(npat):
        for c in flat[int(off[k]):int(off[k + 1])][::-1]:
            s[k], e[k] = oi.lf_map2(np.array([c, c]), np.array([s[k], e[k]]))
            if s[k] == e[k]:
                break
    return s, e, e - s


def check_shape(gi, oi, t):
    import torch
    lib, h, n = gi._lib, gi.handle(), len(t)
    wide = gi.is_wide()
    flat = patterns(t)
    d_flat = torch.from_numpy(flat.view(np.int16) if flat.dtype == np.uint16 else flat).cuda()
    npat = len(LENS)

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a).astype(np.int64)).cuda()

    def outs(k, size=npat):
        return [torch.full((size,), FILL, dtype=torch.int64, device="cuda") for _ in range(k)]

    def finish(rc, bufs, what):
        assert rc == L.OK, (what, rc, lib.fmx_last_error())
        torch.cuda.synchronize()
        assert lib.fmx_stream_status(h) == L.ERR_ARG, what
        assert lib.fmx_stream_status(h) == L.OK, what                  # reading cleared it
        return [b.cpu().numpy().astype(np.uint64) for b in bufs]

    def same(got, want, refused, what):
        for q, (g, w) in enumerate(zip(got, want)):
            for k in range(npat):
                assert int(g[k]) == (0 if k in refused else int(w[k])), (what, q, k, int(g[k]), int(w[k]))

    for variant in VARIANTS:
        off, se, refused = bad_batch(variant, n)
        flat2, off2, se2 = admitted(flat, off, se, refused, n)
        d_off = dev(off)
        d_se = None if se is None else dev(se)
        p_se = None if d_se is None else d_se.data_ptr()
        torch.cuda.synchronize()
        assert lib.fmx_stream_status(h) == L.OK

        what = (variant, "count")
        b = outs(3)
        rc = lib.fmx_count_batch_dev(h, d_flat.data_ptr(), d_off.data_ptr(), npat, p_se, b[0].data_ptr(),
                                     b[1].data_ptr(), b[2].data_ptr(), None)
        same(finish(rc, b, what), expect_count(oi, flat2, off2, se2), refused, what)

        what = (variant, "suffix match")
        b = outs(4)
        rc = lib.fmx_suffix_match_batch_dev(h, d_flat.data_ptr(), d_off.data_ptr(), npat, p_se, 1, b[0].data_ptr(),
                                            b[1].data_ptr(), b[2].data_ptr(), b[3].data_ptr(), None)
        same(finish(rc, b, what), expect_suffix_match(oi, flat2, off2, s0e0=se2), refused, what)
        if wide:
            continue                                                   # (the other two calls refuse a wide handle)

        what = (variant, "mismatch count")
        b = outs(2)
        rc = lib.fmx_mismatch_count_batch_dev(h, d_flat.data_ptr(), d_off.data_ptr(), npat, p_se, 1, b[0].data_ptr(),
                                              b[1].data_ptr(), None)
        same(finish(rc, b, what), expect_mismatch(oi, flat2, off2, s0e0=se2, max_mismatches=1)[:2], refused, what)

        if se is not None:
            continue                                                   # (matching statistics take no start pairs)
        what = (variant, "match stats")
        total = int(off[npat]) - int(off[0])
        b = outs(3, total)
        rc = lib.fmx_match_stats_batch_dev(h, d_flat.data_ptr(), d_off.data_ptr(), npat, total, 1, 0, 0,
                                           b[0].data_ptr(), b[1].data_ptr(), b[2].data_ptr(), None)
        gs, ge, gl = finish(rc, b, what)
        wl, ws, we = expect_match_stats(oi, flat2, off2)
        # slot -> the answers it may hold: those of every admitted pattern that covers it (a pattern that begins inside
        # another shares its slots with it, and either may own them), zeros when no admitted pattern does
        may = [[] for _ in range(total)]
        for k in range(npat):
            if k not in refused:
                for i in range(int(off2[k + 1] - off2[k])):
                    q = int(off2[k]) + i
                    may[int(off[k] - off[0]) + i].append((int(wl[q]), int(ws[q]), int(we[q])))
        assert any(len(m) == 0 for m in may) == (variant == "slice")
        for slot, m in enumerate(may):
            assert (int(gl[slot]), int(gs[slot]), int(ge[slot])) in (m or [(0, 0, 0)]), (what, slot, m)


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_refusals_on_every_kernel_shape(shape, wide):
    gi, text, maxc, kind = SHAPES[shape](wide)
    assert gi.is_wide() == wide
    if shape in ("dna-pair", "dna-both"):
        assert gi.has_pair_index()
    check_shape(gi, oracle(text, maxc, kind), TEXTS[text])
    gi.close()


_FORCED = r"""
import sys
sys.path.insert(0, %r)
sys.path.insert(0, %r)
from fm_index_amd import _lib as L
import test_gpu_pattern_admission as T
assert L.LIB_PATH.endswith("libfmx_measure.so")
done = 0
for shape in T.FORCED:
    for wide in (False, True):
        gi, text, maxc, kind = T.SHAPES[shape](wide)
        T.check_shape(gi, T.oracle(text, maxc, kind), T.TEXTS[text])
        gi.close()
        done += 1
print("forced ok", done)
"""


def test_group_per_pattern_twins_through_the_measurement_build():
    """the group-per-pattern kernels the shipped dispatch never picks for these indexes (a run-length index on
    fmx_count_kernel / fmx_sfx_kernel, every generic wide index on the fmxw_g_* group kernels), forced by the
    measurement build's switches in a process of its own, as tests/test_gpu_suffix_match.py does"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = os.path.join(root, "fm_index_amd", "libfmx_measure.so")
    assert os.path.exists(lib), "fm_index_amd/libfmx_measure.so is missing: run `make -C fm_index_amd/csrc measure`"
    p = subprocess.run([sys.executable, "-c", _FORCED % (root, os.path.join(root, "tests"))],
                       env=dict(os.environ, FMX_LIB=lib, FMX_VARIANT="0", FMXW_R_COUNT_GROUP="1"),
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert p.returncode == 0, p.stderr.decode(errors="replace")[-3000:]
    assert b"forced ok 8" in p.stdout
