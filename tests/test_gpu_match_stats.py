"""Batched matching statistics and SMEM seeds (include/fmx.h: fmx_match_stats_batch / _dev) against the loop of the header
run over the CPU oracle (tests/match_stats_expect.py), through the C ABI with canaries around every output array: one
case per kernel and index kind, the accelerators, min_count / max_len / min_seed_len, a cross-check through
fmx_suffix_match_batch on explicit prefix copies, locate of the seeds, the argument checks and the dev form."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import fm_index_amd as F
from fm_index_amd import _lib as L
from oracle import fm_oracle as O
from match_stats_expect import expect_match_stats
from test_gpu_suffix_match import DNA_KW, abi_match, dna, make_batch, pack, pieces_text, run_text, sym_text

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 5, 255, 256, 257, 1000, 20001]
CANARY = np.uint64(0xC0FFEE0DDBA11)
PAD = 16


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def abi_ms(gi, flat, off, mc=1, max_len=0, msl=0, want=(True, True, True)):
    """fmx_match_stats_batch on host arrays that sit between canaries: (rc, len, s, e); `want` = (len, s, e), an output
    that is not wanted is passed as NULL"""
    flat = np.ascontiguousarray(flat, dtype=gi._dtype)
    off = np.ascontiguousarray(off, dtype=np.uint64)
    npat = len(off) - 1
    total = int(off[-1]) - int(off[0]) if npat else 0
    total = max(total, 0)
    bufs = [np.full(2 * PAD + total, CANARY, dtype=np.uint64) if on else None for on in want]
    views = [None if b is None else b[PAD:] for b in bufs]
    rc = gi._lib.fmx_match_stats_batch(gi.handle(), _ptr(flat), _ptr(off), npat, int(mc), int(max_len), int(msl),
                                       _ptr(views[1]), _ptr(views[2]), _ptr(views[0]))
    for b in bufs:
        if b is not None:
            assert (b[:PAD] == CANARY).all() and (b[len(b) - PAD:] == CANARY).all(), "canary overwritten"
    return (rc,) + tuple(None if b is None else b[PAD:PAD + total] for b in bufs)


def same(got, want, ctx):
    for name, g, w in zip(("len", "s", "e"), got, want):
        assert len(g) == len(w), ctx + (name, len(g), len(w))
        bad = np.nonzero(g != w)[0]
        assert len(bad) == 0, ctx + (name, int(bad[0]), int(g[bad[0]]), int(w[bad[0]]))


def combos(k):
    """(min_count, max_len, min_seed_len): every min_count, every cap around the k-mer length, both seed lengths"""
    return ([(mc, 0, 0) for mc in (0, 1, 2, 5)] + [(1, ml, 0) for ml in (1, 2, k - 1, k, k + 1)] +
            [(1, 0, 1), (1, 0, 3), (2, 0, 3), (5, 0, 1), (2, k, 1), (1, k + 1, 3), (5, 2, 1), (2, k - 1, 3)])


def batch_for(t, maxc, rng, k, per=40):
    """the pattern mix of the suffix-match tests (substrings, one symbol changed, random, with a 0, with a symbol above
    max_character; lengths 0 .. 40) plus substrings of 1, k - 1, k, k + 1 and 40 symbols and two empty patterns"""
    pats, _ = make_batch(t, maxc, rng, per=per)
    n = len(t)
    for m in (1, k - 1, k, k + 1, 40):
        for _ in range(3):
            if 0 < m <= n - 1:
                a = int(rng.integers(0, n - m))
                pats.append(t[a:a + m].copy())
    pats.insert(3, t[:0].copy())
    pats.append(t[:0].copy())
    return pats


def check_index(gi, oi, t, maxc, seed, per=40):
    """every combination of `combos` on the pattern mix; returns the set of lengths seen"""
    rng = np.random.default_rng(seed)
    k = gi.kmer_k() or 4
    flat, off = pack(batch_for(t, maxc, rng, k, per), t.dtype)
    seen = set()
    for mc, ml, msl in combos(k):
        rc, ln, s, e = abi_ms(gi, flat, off, mc, ml, msl)
        assert rc == L.OK, (rc, gi._lib.fmx_last_error())               # out-of-range symbols are no error here
        same((ln, s, e), expect_match_stats(oi, flat, off, mc, ml, msl), (len(t), mc, ml, msl))
        seen |= set(int(x) for x in ln)
    return seen


@pytest.mark.parametrize("variant", ["plain", "pair", "kmer", "both"])
@pytest.mark.parametrize("n", SIZES + [70001])
def test_dna(n, variant):
    """FM over sigma = 4: the one-level kernel, the pair kernel, and both with the k-mer table; the asserts on kmer_k()
    and has_pair_index() keep a case from passing by falling through to another kernel"""
    t = dna(n, 100 + n)
    gi = F.FMIndexWithLocate(F.Text.with_max_character(t, 4), 2, **DNA_KW[variant])
    if variant in ("pair", "both"):
        assert gi.has_pair_index() == (n >= 4)             # (the builder makes none for texts below four symbols)
    else:
        assert not gi.has_pair_index()
    if variant in ("kmer", "both"):
        if n >= 20001:
            assert gi.kmer_k() >= (5 if n == 70001 else 2)
    else:
        assert gi.kmer_k() == 0
    seen = check_index(gi, O.OracleIndex(t, 4), t, 4, 7 * n)
    if n >= 20001:
        kk = gi.kmer_k() or 4
        assert {0, 1, 2, 3, kk - 1, kk, kk + 1} <= seen
    gi.close()


@pytest.mark.parametrize("maxc", [20, 255])
@pytest.mark.parametrize("n", SIZES)
def test_fm_bytes(n, maxc):
    t = sym_text(n, 200 + n + maxc, maxc)
    gi = F.FMIndexWithLocate(F.Text.with_max_character(t, maxc), 2)
    check_index(gi, O.OracleIndex(t, maxc), t, maxc, 11 * n, per=25)
    gi.close()


@pytest.mark.parametrize("n", SIZES)
def test_fm_u16_symbols(n):
    t = sym_text(n, 300 + n, 1000, np.uint16)
    gi = F.FMIndexWithLocate(F.Text.with_max_character(t, 1000), 2)
    assert gi._dtype == np.uint16
    check_index(gi, O.OracleIndex(t, 1000), t, 1000, 13 * n, per=20)
    gi.close()


@pytest.mark.parametrize("text", ["random", "runs"])
@pytest.mark.parametrize("n", SIZES[1:])
def test_rlfm(text, n):
    """random text, and a repetitive text with runs of 64 -- of 1000 at the largest size, longer than the 768 rows a
    record of B spans"""
    if text == "random":
        t, maxc = sym_text(n, 400 + n, 20), 20
    else:
        t, maxc = run_text(n, 500 + n, runlen=1000 if n >= 20001 else 64), 5
    gi = F.RLFMIndexWithLocate(F.Text.with_max_character(t, maxc), 2)
    check_index(gi, O.OracleIndex(t, maxc, kind="rlfm"), t, maxc, 17 * n, per=25)
    gi.close()


@pytest.mark.parametrize("n", SIZES)
def test_multi_pieces(n):
    """lf_map2(0, .) is not monotone there: the pattern mix holds patterns with a 0"""
    t = pieces_text(n, 600 + n)
    gi = F.FMIndexMultiPiecesWithLocate(F.Text.with_max_character(t, 200), 2)
    rng = np.random.default_rng(n)
    pats = batch_for(t, 200, rng, 4, per=25)
    assert any((p == 0).any() for p in pats)
    check_index(gi, O.OracleIndex(t, 200, kind="multi"), t, 200, n, per=25)
    gi.close()


def test_count_only_index_types():
    n = 1000
    t = dna(n, 31)
    gi = F.FMIndex(F.Text.with_max_character(t, 4))
    check_index(gi, O.OracleIndex(t, 4), t, 4, 5)
    gi.close()
    t = sym_text(n, 32, 20)
    gi = F.RLFMIndex(F.Text.with_max_character(t, 20))
    check_index(gi, O.OracleIndex(t, 20, kind="rlfm"), t, 20, 6)
    gi.close()
    t = pieces_text(n, 33)
    gi = F.FMIndexMultiPieces(F.Text.with_max_character(t, 200))
    check_index(gi, O.OracleIndex(t, 200, kind="multi"), t, 200, 7)
    gi.close()


def test_accelerators_change_nothing():
    """plain, pair index, k-mer table, both and the builder's own choice give identical arrays on one text"""
    n = 70001
    t = dna(n, 41)
    tx = F.Text.with_max_character(t, 4)
    idx = {v: F.FMIndexWithLocate(tx, 2, **kw) for v, kw in DNA_KW.items()}
    assert idx["both"].has_pair_index() and idx["both"].kmer_k() >= 5 and idx["kmer"].kmer_k() >= 5
    k = idx["both"].kmer_k()
    flat, off = pack(batch_for(t, 4, np.random.default_rng(4), k, per=60), np.uint8)
    for mc, ml, msl in combos(k):
        want = abi_ms(idx["plain"], flat, off, mc, ml, msl)
        assert want[0] == L.OK
        for v in ("pair", "kmer", "both", "auto"):
            got = abi_ms(idx[v], flat, off, mc, ml, msl)
            assert got[0] == L.OK
            same(got[1:], want[1:], (v, mc, ml, msl))
    for gi in idx.values():
        gi.close()


def test_cross_check_through_suffix_match_on_prefix_copies():
    """independent of the oracle: fmx_suffix_match_batch on a copy of every prefix gives the same (s, e, L) wherever
    L > 0 (an empty match is the start pair there and (0, 0) here)"""
    n = 20001
    t = dna(n, 51)
    for gi in (F.FMIndexWithLocate(F.Text.with_max_character(t, 4), 2),
               F.RLFMIndexWithLocate(F.Text.with_max_character(t, 4), 2)):
        pats = batch_for(t, 4, np.random.default_rng(9), gi.kmer_k() or 4, per=20)
        flat, off = pack(pats, np.uint8)
        pflat, poff = pack([p[:i] for p in pats for i in range(1, len(p) + 1)], np.uint8)
        for mc in (1, 2, 5):
            rc, ln, s, e = abi_ms(gi, flat, off, mc)
            rc2, ss, se, sc, sl = abi_match(gi, pflat, poff, min_count=mc)
            assert rc == L.OK and rc2 == L.OK and len(ln) == len(sl)
            assert (ln == sl).all()
            hit = ln > 0
            assert hit.any() and (~hit).any()
            assert (s[hit] == ss[hit]).all() and (e[hit] == se[hit]).all()
            assert not s[~hit].any() and not e[~hit].any()
        gi.close()


def test_locate_of_the_seeds_gives_the_windows():
    n = 20001
    t = dna(n, 81)
    gi = F.FMIndexWithLocate(F.Text.with_max_character(t, 4), 2)
    rng = np.random.default_rng(8)
    pats = []
    for q in range(30):
        m = int(rng.integers(12, 41))
        a = int(rng.integers(0, n - 1 - m))
        p = t[a:a + m].copy()
        for _ in range(q % 3):
            p[int(rng.integers(0, m))] = rng.integers(1, 5)
        pats.append(p)
    b = gi.match_stats_many(patterns=pats, min_seed_len=8)
    assert isinstance(b, F.MatchStatsBatch) and len(b.lengths) == sum(len(p) for p in pats)
    sd = b.seeds()
    hoff, pos = b.locate()
    assert len(sd) >= len(pats) and len(hoff) == len(sd) + 1
    for j, q in enumerate(sd):
        p = pats[int(q["pattern"])]
        w = p[int(q["begin"]):int(q["begin"]) + int(q["length"])]
        assert int(q["length"]) >= 8
        win = np.lib.stride_tricks.sliding_window_view(t, len(w))
        want = np.nonzero((win == w[None, :]).all(axis=1))[0]
        mine = np.sort(pos[int(hoff[j]):int(hoff[j + 1])].astype(np.int64))
        assert (mine == want).all() and len(mine) == int(q["e"] - q["s"]), j
    gi.close()


@pytest.mark.parametrize("n,max_len", [(1000, 0), (20001, 64)])
def test_pattern_equal_to_the_whole_text(n, max_len):
    """every prefix of the text occurs: L[i] = i uncapped (O(m^2) steps, so n = 1000), min(i, 64) with the cap"""
    t = dna(n, 61)
    oi = O.OracleIndex(t, 4)
    flat, off = pack([t[:-1]], np.uint8)
    i = np.arange(1, n, dtype=np.uint64)
    for kw in (dict(plain=True), dict(pair_index=True, kmer_table=True)):
        gi = F.FMIndexWithLocate(F.Text.with_max_character(t, 4), 2, **kw)
        for msl in (0, 3):
            rc, ln, s, e = abi_ms(gi, flat, off, 1, max_len, msl)
            assert rc == L.OK
            assert (ln == (np.minimum(i, np.uint64(max_len)) if max_len else i)).all()
            same((ln, s, e), expect_match_stats(oi, flat, off, 1, max_len, msl), (n, max_len, msl))
        gi.close()


def _group_cap():
    """groups of the largest grid fmx_grid_for_groups gives, read from the source"""
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(here, "fm_index_amd", "csrc")
    src = open(os.path.join(csrc, "fmx_query.hip")).read() + open(os.path.join(csrc, "fmx_device.h")).read() + \
        open(os.path.join(csrc, "fmx_internal.h")).read()
    val = {nm: int(re.search(r"#define\s+%s\s+(\d+)" % nm, src).group(1)) for nm in ("FMX_BLOCK", "FMX_MAX_BLOCKS",
                                                                                   "FMX_GROUP")}
    return val["FMX_MAX_BLOCKS"] * val["FMX_BLOCK"] // val["FMX_GROUP"]


def test_more_slots_than_groups():
    """a batch in which every group takes more than two slots, and not the same number each"""
    cap = _group_cap()
    assert cap >= 1024
    n = 1 << 16
    t = dna(n, 61)
    oi = O.OracleIndex(t, 4)
    m = 19
    npat = (2 * cap + 12345) // m + 1
    assert (npat * m) % cap != 0 and npat * m > 2 * cap
    rng = np.random.default_rng(12)
    a = rng.integers(0, n - 1 - m, npat)
    mat = t[a[:, None] + np.arange(m)[None, :]].copy()
    hit = rng.integers(0, 3, npat) > 0
    mat[np.nonzero(hit)[0], rng.integers(0, m, int(hit.sum()))] = rng.integers(1, 5, int(hit.sum()))
    flat = np.ascontiguousarray(mat.reshape(-1))
    off = np.arange(npat + 1, dtype=np.uint64) * np.uint64(m)
    for kw in (dict(plain=True), dict(pair_index=True, kmer_table=True)):
        gi = F.FMIndexWithLocate(F.Text.with_max_character(t, 4), 2, **kw)
        for mc, ml, msl in ((1, 0, 0), (2, 0, 5)):
            rc, ln, s, e = abi_ms(gi, flat, off, mc, ml, msl)
            assert rc == L.OK
            same((ln, s, e), expect_match_stats(oi, flat, off, mc, ml, msl), (mc, ml, msl))
        gi.close()


# ---- the dev form: torch tensors between canaries ----
def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).cuda()


class DevOut:
    """three device arrays of `cap` entries, every entry and PAD entries before and after preset to CANARY"""

    def __init__(self, cap, want=(True, True, True)):
        import torch
        self.cap = cap
        self.t = [torch.from_numpy(np.full(2 * PAD + cap, CANARY, dtype=np.uint64).view(np.int64)).cuda() if on else None
                  for on in want]

    def ptr(self, j):
        return None if self.t[j] is None else self.t[j].data_ptr() + 8 * PAD

    def read(self):
        out = []
        for x in self.t:
            if x is None:
                out.append(None)
                continue
            b = x.cpu().numpy().view(np.uint64)
            assert (b[:PAD] == CANARY).all() and (b[len(b) - PAD:] == CANARY).all(), "canary overwritten"
            out.append(b[PAD:PAD + self.cap])
        return out


def dev_ms(gi, d_flat, d_off, npat, total, mc=1, max_len=0, msl=0, out=None, stream=None):
    """fmx_match_stats_batch_dev + synchronise: (rc, status, len, s, e)"""
    import torch
    out = out or DevOut(total)
    torch.cuda.synchronize()
    rc = gi._lib.fmx_match_stats_batch_dev(gi.handle(), d_flat.data_ptr(), None if d_off is None else d_off.data_ptr(),
                                           npat, total, int(mc), int(max_len), int(msl), out.ptr(1), out.ptr(2),
                                           out.ptr(0), None if stream is None else stream.cuda_stream)
    torch.cuda.synchronize()
    status = gi._lib.fmx_stream_status(gi.handle())
    return (rc, status) + tuple(out.read())


def test_errors():
    n = 20001
    t = dna(n, 95)
    tx = F.Text.with_max_character(t, 4)
    gi = F.FMIndexWithLocate(tx, 2)
    oi = O.OracleIndex(t, 4)
    pats = batch_for(t, 4, np.random.default_rng(1), gi.kmer_k() or 4, per=20)
    flat, off = pack(pats, np.uint8)
    npat, total = len(pats), int(off[-1])
    wl, ws, we = expect_match_stats(oi, flat, off)
    rc, ln, s, e = abi_ms(gi, flat, off)
    assert rc == L.OK
    same((ln, s, e), (wl, ws, we), ("ok",))
    # out_s / out_e may be NULL, alone and together; with the seed filter asked for as well
    for want in ((True, False, True), (True, True, False), (True, False, False)):
        for msl in (0, 3):
            w3 = expect_match_stats(oi, flat, off, 1, 0, msl)
            rc, l2, s2, e2 = abi_ms(gi, flat, off, 1, 0, msl, want=want)
            assert rc == L.OK and (l2 == w3[0]).all()
            assert s2 is None or (s2 == w3[1]).all()
            assert e2 is None or (e2 == w3[2]).all()
    # NULL out_len: refused before anything is launched
    rc, none, s2, e2 = abi_ms(gi, flat, off, want=(False, True, True))
    assert rc == L.ERR_ARG and (s2 == CANARY).all() and (e2 == CANARY).all()
    d_flat, d_off = _dev(flat), _dev(off)
    o = DevOut(total, want=(False, True, True))
    rc, st, none, s2, e2 = dev_ms(gi, d_flat, d_off, npat, total, out=o)
    assert rc == L.ERR_ARG and st == L.OK and (s2 == CANARY).all() and (e2 == CANARY).all()

    def owned(boff, valid):
        """expected arrays for offsets `boff` (slots relative to boff[0]) when only the patterns `valid` count"""
        el, es, ee = (np.zeros(total, dtype=np.uint64) for _ in range(3))
        for k in valid:
            a, b = int(boff[k]), int(boff[k + 1])
            pl, ps, pe = expect_match_stats(oi, flat, np.array([a, b], dtype=np.uint64))
            lo = a - int(boff[0])
            el[lo:lo + b - a], es[lo:lo + b - a], ee[lo:lo + b - a] = pl, ps, pe
        return el, es, ee

    kb = int(np.nonzero((off[1:-2] > off[0] + 1) & (off[2:-1] > off[1:-2]))[0][2]) + 1   # a non-empty pattern in the middle
    # offsets going backwards at pattern kb: it is never read; the next pattern starts one symbol early and is valid
    boff = off.copy()
    boff[kb + 1] = off[kb] - np.uint64(1)
    rc, l2, s2, e2 = abi_ms(gi, flat, boff)
    assert rc == L.ERR_ARG
    a, b = int(off[kb]), int(off[kb + 2])
    el, es, ee = owned(boff, [kb + 1])
    assert (l2[:a - 1] == wl[:a - 1]).all() and (l2[b:] == wl[b:]).all() and (l2[a:b] == el[a:b]).all()
    assert (s2[:a - 1] == ws[:a - 1]).all() and (s2[b:] == ws[b:]).all() and (s2[a:b] == es[a:b]).all()
    assert (e2[:a - 1] == we[:a - 1]).all() and (e2[b:] == we[b:]).all() and (e2[a:b] == ee[a:b]).all()
    assert (int(l2[a - 1]), int(s2[a - 1]), int(e2[a - 1])) in ((int(wl[a - 1]), int(ws[a - 1]), int(we[a - 1])),
                                                                 (int(el[a - 1]), int(es[a - 1]), int(ee[a - 1])))
    # beyond pat_off[npat]: pattern kb leaves the buffer and pattern kb + 1 goes backwards; neither is read
    boff = off.copy()
    boff[kb + 1] = off[-1] + np.uint64(5)
    rc, l2, s2, e2 = abi_ms(gi, flat, boff)
    assert rc == L.ERR_ARG
    keep = np.ones(total, dtype=bool)
    keep[a:b] = False
    assert (l2[keep] == wl[keep]).all() and (s2[keep] == ws[keep]).all() and (e2[keep] == we[keep]).all()
    assert not l2[a:b].any() and not s2[a:b].any() and not e2[a:b].any()
    # below pat_off[0]: a slice with absolute offsets whose second offset falls below the first
    k0 = 5
    sl = off[k0:].copy()
    lo = int(sl[0])
    assert lo > 0 and int(off[k0 + 2]) > lo
    sl[1] = sl[0] - np.uint64(1)
    rc, l2, s2, e2 = abi_ms(gi, flat, sl)
    assert rc == L.ERR_ARG
    b = int(off[k0 + 2]) - lo
    assert (l2[b:] == wl[lo + b:]).all() and (s2[b:] == ws[lo + b:]).all() and (e2[b:] == we[lo + b:]).all()
    assert not l2[:b].any() and not s2[:b].any() and not e2[:b].any()
    # total_syms too small: reported, nothing at or above it written; too large: the extra slots are zero
    for msl in (0, 3):
        w3 = expect_match_stats(oi, flat, off, 1, 0, msl)
        cut = total - 7
        o = DevOut(total)
        o.cap = total
        rc, st, l2, s2, e2 = dev_ms(gi, d_flat, d_off, npat, cut, msl=msl, out=o)
        assert rc == L.OK and st == L.ERR_ARG
        assert (l2[:cut] == w3[0][:cut]).all() and (l2[cut:] == CANARY).all()
        assert (s2[cut:] == CANARY).all() and (e2[cut:] == CANARY).all()
        if msl == 0:
            assert (s2[:cut] == w3[1][:cut]).all() and (e2[:cut] == w3[2][:cut]).all()
        rc, st, l2, s2, e2 = dev_ms(gi, d_flat, d_off, npat, total + 9, msl=msl)
        assert rc == L.OK and st == L.ERR_ARG
        same((l2[:total], s2[:total], e2[:total]), w3, ("long", msl))
        assert not l2[total:].any() and not s2[total:].any() and not e2[total:].any()
    # npat == 0 with slots: no pattern owns them
    rc, st, l2, s2, e2 = dev_ms(gi, d_flat, None, 0, 11)
    assert rc == L.ERR_ARG and not l2.any() and not s2.any() and not e2.any()
    gi.close()
    # a handle of the wide engine: FMX_ERR_UNSUPPORTED with a message, outputs untouched
    gw = F.FMIndexWithLocate(tx, 2, force_wide=True)
    assert gw.is_wide()
    rc, l2, s2, e2 = abi_ms(gw, flat, off)
    assert rc == L.ERR_UNSUPPORTED and (l2 == CANARY).all() and (s2 == CANARY).all() and (e2 == CANARY).all()
    assert b"64-bit" in gw._lib.fmx_last_error()
    rc, st, l2, s2, e2 = dev_ms(gw, d_flat, d_off, npat, total)
    assert rc == L.ERR_UNSUPPORTED and (l2 == CANARY).all() and (s2 == CANARY).all() and (e2 == CANARY).all()
    with pytest.raises(F.Error) as ei:
        gw.match_stats_many(patterns=[b"\x01\x02"])
    assert ei.value.code == L.ERR_UNSUPPORTED
    gw.close()


def test_empty_text_no_patterns_and_empty_patterns():
    gi = F.FMIndex(F.Text(b""))
    flat, off = pack([np.array(p, dtype=np.uint8) for p in ([1], [], [1, 2], [0])], np.uint8)
    for msl in (0, 1):
        rc, ln, s, e = abi_ms(gi, flat, off, msl=msl)
        assert rc == L.OK and len(ln) == 4 and not ln.any() and not s.any() and not e.any()
    boff = off.copy()
    boff[2] = 0
    rc, ln, s, e = abi_ms(gi, flat, boff)
    assert rc == L.ERR_ARG and not ln.any() and not s.any() and not e.any()
    gi.close()
    t = dna(1000, 5)
    gi = F.FMIndexWithLocate(F.Text.with_max_character(t, 4), 2)
    for pats in ([], [t[:0]], [t[:0], t[:0], t[:0]]):
        flat, off = pack(pats, np.uint8)
        rc, ln, s, e = abi_ms(gi, flat, off, msl=1)
        assert rc == L.OK and len(ln) == 0
    d_flat, d_off = _dev(flat), _dev(off)
    rc, st, ln, s, e = dev_ms(gi, d_flat, d_off, 3, 0, out=DevOut(0))
    assert rc == L.OK and st == L.OK
    rc, st, ln, s, e = dev_ms(gi, d_flat, None, 0, 0, out=DevOut(0))
    assert rc == L.OK and st == L.OK
    b = gi.match_stats_many(patterns=[])
    assert len(b.lengths) == 0 and len(b.seeds()) == 0 and b.offsets.tolist() == [0]
    gi.close()


def test_dev_form_on_a_stream_twice_into_the_same_arrays():
    """resident patterns, a non-default stream, the status through fmx_stream_status(); the second call finds the first
    call's results in the arrays (not the canaries) and gives the same"""
    import torch
    n = 20001
    t = dna(n, 77)
    oi = O.OracleIndex(t, 4)
    st = torch.cuda.Stream()
    for gi in (F.FMIndexWithLocate(F.Text.with_max_character(t, 4), 2),
               F.RLFMIndexWithLocate(F.Text.with_max_character(t, 4), 2)):
        pats = batch_for(t, 4, np.random.default_rng(3), gi.kmer_k() or 4, per=30)
        flat, off = pack(pats, np.uint8)
        npat, total = len(pats), int(off[-1])
        d_flat, d_off = _dev(flat), _dev(off)
        for mc, ml, msl in ((1, 0, 0), (2, 0, 3), (1, 5, 5)):
            want = expect_match_stats(oi, flat, off, mc, ml, msl)
            o = DevOut(total)
            for _ in range(2):
                rc, status, ln, s, e = dev_ms(gi, d_flat, d_off, npat, total, mc, ml, msl, out=o, stream=st)
                assert rc == L.OK and status == L.OK
                same((ln, s, e), want, (mc, ml, msl))
        gi.close()


def test_python_mississippi():
    index = F.FMIndexWithLocate(F.Text(b"mississippi\x00"), 2)
    b = index.match_stats_many([b"sispi", b"", b"ssi"])
    assert b.offsets.tolist() == [0, 5, 5, 8] and b.lengths.tolist() == [1, 2, 3, 1, 2, 1, 2, 3]
    assert len(b.seeds()) == 8                                        # no filter: every non-empty slot
    b = index.match_stats_many([b"sispi", b"", b"ssi"], min_seed_len=1)
    assert b.lengths.tolist() == [1, 2, 3, 1, 2, 1, 2, 3]
    sd = b.seeds()
    assert [(int(q["pattern"]), int(q["begin"]), int(q["length"])) for q in sd] == [(0, 0, 3), (0, 3, 2), (2, 0, 3)]
    assert [(int(q["s"]), int(q["e"])) for q in sd] == [(9, 10), (6, 7), (10, 12)]    # sis, pi, ssi
    hoff, pos = b.locate()
    assert [sorted(pos[int(hoff[j]):int(hoff[j + 1])].tolist()) for j in range(3)] == [[3], [9], [2, 5]]
    b = index.match_stats_many([b"sispi"], min_seed_len=3)
    assert [(int(q["begin"]), int(q["length"])) for q in b.seeds()] == [(0, 3)]
    b = index.match_stats_many([b"sispi"], max_len=2)
    assert b.lengths.tolist() == [1, 2, 2, 1, 2]
    index.close()
