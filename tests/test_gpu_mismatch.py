"""Batched backward search with up to two mismatches (include/fmx.h: fmx_mismatch_count_batch / fmx_mismatch_search_batch
and their _dev forms) against the enumeration of the header run over the CPU oracle (tests/mismatch_expect.py), through
the C ABI: every index kind of the 32-bit engine, K = 0 / 1 / 2, the accelerators, an independent cross-check through
fmx_count_batch on the enumerated variants, refinement, locate, the safety of pass 2 and the argument checks."""
import ctypes as C

import numpy as np
import pytest

import fm_index_amd as F
from fm_index_amd import _lib as L
from oracle import fm_oracle as O
from mismatch_expect import UNUSED, expect_mismatch, variants
from test_gpu_suffix_match import abi_count, dna, make_batch, pack, pieces_text, run_text, sym_text

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 5, 255, 256, 257, 1000, 20001]
CANARY = np.uint64(0xC0FFEE0DDBA11)
PAD = 16


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _prep(gi, flat, off, s0e0):
    flat = np.ascontiguousarray(flat, dtype=gi._dtype)
    off = np.ascontiguousarray(off, dtype=np.uint64)
    se = None if s0e0 is None else np.ascontiguousarray(s0e0, dtype=np.uint64)
    return flat, off, len(off) - 1, se


def abi_pass1(gi, flat, off, s0e0=None, K=1, want=(True, True)):
    """fmx_mismatch_count_batch on host arrays: (rc, nint, count)"""
    flat, off, npat, se = _prep(gi, flat, off, s0e0)
    outs = [np.full(max(npat, 1), 0xDEAD, dtype=np.uint64) if w else None for w in want]
    rc = gi._lib.fmx_mismatch_count_batch(gi.handle(), _ptr(flat), _ptr(off), npat, _ptr(se), K, *[_ptr(o) for o in outs])
    return (rc,) + tuple(None if o is None else o[:npat] for o in outs)


def abi_pass2(gi, flat, off, ooff, total, s0e0=None, K=1, want=(True, True, True), cap=None):
    """fmx_mismatch_search_batch on host arrays that sit between canaries: (rc, s, e, edit); `cap` = entries the
    arrays really have (default `total`), every one preset to CANARY like the PAD entries before and after"""
    flat, off, npat, se = _prep(gi, flat, off, s0e0)
    ooff = np.ascontiguousarray(ooff, dtype=np.uint64)
    cap = total if cap is None else cap
    bufs = [np.full(2 * PAD + w * max(cap, 1), CANARY, dtype=np.uint64) if on else None
            for w, on in zip((1, 1, 2), want)]
    views = [None if b is None else b[PAD:] for b in bufs]
    rc = gi._lib.fmx_mismatch_search_batch(gi.handle(), _ptr(flat), _ptr(off), npat, _ptr(se), K, _ptr(ooff), total,
                                           *[_ptr(v) for v in views])
    for b in bufs:
        if b is not None:
            assert (b[:PAD] == CANARY).all() and (b[len(b) - PAD:] == CANARY).all(), "canary overwritten"
    return (rc,) + tuple(None if b is None else b[PAD:PAD + w * cap] for b, w in zip(bufs, (1, 1, 2)))


def scan(nint):
    o = np.zeros(len(nint) + 1, dtype=np.uint64)
    o[1:] = np.cumsum(nint, dtype=np.uint64)
    return o


def search(gi, flat, off, s0e0=None, K=1):
    """both passes and the scan: (nint, count, s, e, edit)"""
    rc, nint, count = abi_pass1(gi, flat, off, s0e0, K)
    assert rc == L.OK, (rc, gi._lib.fmx_last_error())
    ooff = scan(nint)
    rc, s, e, ed = abi_pass2(gi, flat, off, ooff, int(ooff[-1]), s0e0, K)
    assert rc == L.OK, (rc, gi._lib.fmx_last_error())
    return nint, count, s, e, ed


def same(got, want, ctx):
    for name, g, w in zip(("nint", "count", "s", "e", "edit"), got, want):
        assert len(g) == len(w), ctx + (name, len(g), len(w))
        bad = np.nonzero(g != w)[0]
        assert len(bad) == 0, ctx + (name, int(bad[0]), int(g[bad[0]]), int(w[bad[0]]))


def nedits(ed):
    return (ed.reshape(-1, 2) != UNUSED).sum(axis=1)


def check_index(gi, oi, t, maxc, seed, per=14):
    """K = 0, 1, 2 on the pattern mix; returns the set of edit counts seen"""
    rng = np.random.default_rng(seed)
    pats, _ = make_batch(t, maxc, rng, per=per, mmax=24)
    flat, off = pack(pats, t.dtype)
    seen = set()
    for K in (0, 1, 2):
        got = search(gi, flat, off, K=K)
        same(got, expect_mismatch(oi, flat, off, max_mismatches=K), (len(t), K))
        seen |= set(int(x) for x in nedits(got[4]))
    return seen


DNA_N = SIZES + [70001]


@pytest.mark.parametrize("n", DNA_N)
def test_dna_one_level(n):
    """FMIndex over sigma = 4: the one-level kernel; 70001 crosses 2^16 rows"""
    t = dna(n, 100 + n)
    gi = F.FMIndexWithLocate(F.Text.with_max_character(t, 4), 2, plain=True)
    seen = check_index(gi, O.OracleIndex(t, 4), t, 4, 7 * n)
    if n >= 1000:
        assert seen == {0, 1, 2}
    gi.close()


@pytest.mark.parametrize("n", SIZES)
def test_fm_bytes_max_character_20(n):
    t = sym_text(n, 200 + n, 20)
    gi = F.FMIndexWithLocate(F.Text.with_max_character(t, 20), 2)
    seen = check_index(gi, O.OracleIndex(t, 20), t, 20, 11 * n)
    if n >= 1000:
        assert seen == {0, 1, 2}
    gi.close()


@pytest.mark.parametrize("n", SIZES)
def test_fm_bytes_max_character_255(n):
    """the whole byte alphabet, about 30 patterns"""
    t = sym_text(n, 250 + n, 255)
    gi = F.FMIndexWithLocate(F.Text.with_max_character(t, 255), 2)
    seen = check_index(gi, O.OracleIndex(t, 255), t, 255, 23 * n, per=9)
    if n >= 1000:
        assert seen == {0, 1, 2}
    gi.close()


@pytest.mark.parametrize("n", SIZES)
def test_fm_u16_symbols(n):
    t = sym_text(n, 300 + n, 1000, np.uint16)
    gi = F.FMIndexWithLocate(F.Text.with_max_character(t, 1000), 2)
    assert gi._dtype == np.uint16
    seen = check_index(gi, O.OracleIndex(t, 1000), t, 1000, 13 * n, per=6)
    if n >= 20001:
        assert seen == {0, 1, 2}
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
    seen = check_index(gi, O.OracleIndex(t, maxc, kind="rlfm"), t, maxc, 17 * n)
    if n >= 1000 and text == "random":
        assert seen == {0, 1, 2}
    gi.close()


@pytest.mark.parametrize("n", SIZES)
def test_multi_pieces(n):
    t = pieces_text(n, 600 + n)
    gi = F.FMIndexMultiPiecesWithLocate(F.Text.with_max_character(t, 200), 2)
    seen = check_index(gi, O.OracleIndex(t, 200, kind="multi"), t, 200, 19 * n, per=9)
    if n >= 1000:
        assert seen == {0, 1, 2}
    gi.close()


def test_fm_without_locate_and_rlfm_without_locate():
    n = 1000
    t = dna(n, 31)
    gi = F.FMIndex(F.Text.with_max_character(t, 4))
    check_index(gi, O.OracleIndex(t, 4), t, 4, 5)
    gi.close()
    t = sym_text(n, 32, 20)
    gi = F.RLFMIndex(F.Text.with_max_character(t, 20))
    check_index(gi, O.OracleIndex(t, 20, kind="rlfm"), t, 20, 6)
    gi.close()


def test_accelerators_change_nothing():
    """the default DNA index (pair index and k-mer table) and FMX_FLAG_PLAIN give identical arrays"""
    n = 70001
    t = dna(n, 41)
    tx = F.Text.with_max_character(t, 4)
    plain = F.FMIndexWithLocate(tx, 2, plain=True)
    both = F.FMIndexWithLocate(tx, 2, pair_index=True, kmer_table=True)
    auto = F.FMIndexWithLocate(tx, 2)
    assert both.has_pair_index() and both.kmer_k() >= 2
    pats, _ = make_batch(t, 4, np.random.default_rng(4), per=40, mmax=24)
    flat, off = pack(pats, np.uint8)
    for K in (0, 1, 2):
        want = search(plain, flat, off, K=K)
        for gi in (both, auto):
            same(search(gi, flat, off, K=K), want, (K,))
    for gi in (plain, both, auto):
        gi.close()


def test_cross_check_through_count_on_every_variant():
    """independent of the oracle: every variant enumerated on the host in the stated order, fmx_count_batch on them;
    the non-empty results, in order, are pass 2's"""
    n = 20001
    t = dna(n, 51)
    gi = F.FMIndexWithLocate(F.Text.with_max_character(t, 4), 2)
    rng = np.random.default_rng(9)
    pats, _ = make_batch(t, 4, rng, per=10, mmax=24)
    pats = [p for p in pats if len(p) <= 16]
    flat, off = pack(pats, np.uint8)
    for K in (1, 2):
        nint, count, s, e, ed = search(gi, flat, off, K=K)
        ooff = scan(nint)
        vs = [variants(p, 4, K) for p in pats]
        vflat, voff = pack([v for per_p in vs for v, _ in per_p], np.uint8)
        rc, cs, ce, cc = abi_count(gi, vflat, voff)
        assert rc == L.OK
        at = 0
        for k, per_p in enumerate(vs):
            hit = np.nonzero(cc[at:at + len(per_p)] > 0)[0]
            a, b = int(ooff[k]), int(ooff[k + 1])
            assert b - a == len(hit), (K, k)
            assert (s[a:b] == cs[at + hit]).all() and (e[a:b] == ce[at + hit]).all(), (K, k)
            words = [[(q << 32) | c for q, c in per_p[j][1]] + [int(UNUSED)] * (2 - len(per_p[j][1])) for j in hit]
            assert ed[2 * a:2 * b].tolist() == [w for ws in words for w in ws], (K, k)
            assert int(count[k]) == int(cc[at + hit].sum())
            at += len(per_p)
    gi.close()


def test_budget_zero_is_count():
    """K = 0: nint == (count > 0), and (s, e, count) of fmx_count_batch on the patterns without out-of-range symbols"""
    n = 20001
    t = dna(n, 61)
    gi = F.FMIndexWithLocate(F.Text.with_max_character(t, 4), 2)
    pats, _ = make_batch(t, 4, np.random.default_rng(2), per=60, mmax=24)
    flat, off = pack(pats, np.uint8)
    nint, count, s, e, ed = search(gi, flat, off, K=0)
    assert (nint == (count > 0)).all() and (ed == UNUSED).all()
    inr = [k for k, p in enumerate(pats) if len(p) == 0 or int(p.max()) <= 4]
    assert len(inr) < len(pats)
    f2, o2 = pack([pats[k] for k in inr], np.uint8)
    rc, cs, ce, cc = abi_count(gi, f2, o2)
    assert rc == L.OK and (count[inr] == cc).all()
    ooff = scan(nint)
    for q, k in enumerate(inr):
        if cc[q]:
            assert (int(s[ooff[k]]), int(e[ooff[k]])) == (int(cs[q]), int(ce[q]))
    out = [k for k in range(len(pats)) if k not in set(inr)]
    assert not count[out].any() and not nint[out].any()
    gi.close()


def test_refinement_from_a_right_hand_part():
    """a second call with s0e0 from a count of the right-hand part gives what the whole pattern gives with its
    substitutions in the left part; pos is relative to the shorter pattern"""
    n = 20001
    t = dna(n, 71)
    gi = F.FMIndexWithLocate(F.Text.with_max_character(t, 4), 2)
    oi = O.OracleIndex(t, 4)
    rng = np.random.default_rng(3)
    starts = rng.integers(0, n - 30, 60)
    whole = [t[a:a + 20].copy() for a in starts]
    for p in whole[::2]:
        p[int(rng.integers(0, 12))] = rng.integers(1, 5)
    left, right = [p[:12] for p in whole], [p[12:] for p in whole]
    rf, ro = pack(right, np.uint8)
    rc, rs, re, rcnt = abi_count(gi, rf, ro)
    assert rc == L.OK and (rcnt > 0).all()
    se = np.stack([rs, re], axis=1).reshape(-1)
    lf, lo = pack(left, np.uint8)
    wf, wo = pack(whole, np.uint8)
    for K in (1, 2):
        got = search(gi, lf, lo, s0e0=se, K=K)
        same(got, expect_mismatch(oi, lf, lo, s0e0=se, max_mismatches=K), (K,))
        full = search(gi, wf, wo, K=K)
        # the whole pattern's intervals whose substitutions all lie in the left part (pos < 12), in order
        fo = scan(full[0])
        pos = np.where(full[4] == UNUSED, np.uint64(0), full[4] >> np.uint64(32)).reshape(-1, 2)
        inleft = (pos < 12).all(axis=1)
        at = 0
        for k in range(len(whole)):
            sel = np.nonzero(inleft[int(fo[k]):int(fo[k + 1])])[0] + int(fo[k])
            m = int(got[0][k])
            assert m == len(sel)
            assert (got[2][at:at + m] == full[2][sel]).all() and (got[3][at:at + m] == full[3][sel]).all()
            assert (got[4].reshape(-1, 2)[at:at + m] == full[4].reshape(-1, 2)[sel]).all()
            at += m
    gi.close()


def test_locate_gives_the_windows_within_the_distance():
    n = 20001
    t = dna(n, 81)
    gi = F.FMIndexWithLocate(F.Text.with_max_character(t, 4), 2)
    rng = np.random.default_rng(8)
    pats = []
    for q in range(40):
        m = int(rng.integers(6, 25))
        a = int(rng.integers(0, n - 1 - m))
        p = t[a:a + m].copy()
        for _ in range(q % 3):
            p[int(rng.integers(0, m))] = rng.integers(1, 5)
        pats.append(p)
    for K in (1, 2):
        b = gi.mismatch_search_many(patterns=pats, max_mismatches=K)
        assert isinstance(b, F.MismatchBatch) and len(b.nint) == len(pats) and b.edits.shape == (len(b.s), 2)
        hoff, pos = b.locate()
        for k, p in enumerate(pats):
            mine = np.sort(pos[int(hoff[int(b.off[k])]):int(hoff[int(b.off[k + 1])])].astype(np.int64))
            win = np.lib.stride_tricks.sliding_window_view(t, len(p))
            diff = win != p[None, :]
            want = np.nonzero((diff.sum(axis=1) <= K) & ~(diff & (win == 0)).any(axis=1))[0]
            assert (mine == want).all() and len(mine) == int(b.counts[k]), (K, k)
    gi.close()


def test_pass_two_is_safe_against_offsets_that_do_not_fit():
    """offsets one slot short for one pattern, one slot long, a total_intervals that is too small: FMX_ERR_ARG, the
    canaries intact, nothing written outside a pattern's own slots; each output NULL in turn"""
    n = 20001
    t = dna(n, 91)
    for gi in (F.FMIndexWithLocate(F.Text.with_max_character(t, 4), 2),
               F.RLFMIndexWithLocate(F.Text.with_max_character(t, 4), 2)):
        pats, _ = make_batch(t, 4, np.random.default_rng(6), per=30, mmax=24)
        flat, off = pack(pats, np.uint8)
        K = 1
        nint, count, s, e, ed = search(gi, flat, off, K=K)
        ooff = scan(nint)
        total = int(ooff[-1])
        kb = int(np.nonzero(nint >= 2)[0][3])                       # a pattern with two intervals or more, not the first
        for want in ((False, True, True), (True, False, True), (True, True, False), (False, False, False)):
            rc, s2, e2, ed2 = abi_pass2(gi, flat, off, ooff, total, K=K, want=want)
            assert rc == L.OK
            assert s2 is None or (s2 == s).all()
            assert e2 is None or (e2 == e).all()
            assert ed2 is None or (ed2 == ed).all()
        a, b = int(ooff[kb]), int(ooff[kb + 1])
        # one slot short: pattern kb has b - a - 1 slots, everything behind it moves down by one
        short = ooff.copy()
        short[kb + 1:] -= np.uint64(1)
        rc, s2, e2, ed2 = abi_pass2(gi, flat, off, short, total - 1, K=K, cap=total)
        assert rc == L.ERR_ARG
        assert (s2[:b - 1] == s[:b - 1]).all() and (s2[b - 1:total - 1] == s[b:]).all() and s2[total - 1] == CANARY
        assert (e2[:b - 1] == e[:b - 1]).all() and (e2[b - 1:total - 1] == e[b:]).all() and e2[total - 1] == CANARY
        assert (ed2[:2 * (b - 1)] == ed[:2 * (b - 1)]).all() and (ed2[2 * (b - 1):2 * (total - 1)] == ed[2 * b:]).all()
        # one slot long: the extra slot of pattern kb stays as it was
        long_ = ooff.copy()
        long_[kb + 1:] += np.uint64(1)
        rc, s2, e2, ed2 = abi_pass2(gi, flat, off, long_, total + 1, K=K)
        assert rc == L.ERR_ARG
        assert (s2[:b] == s[:b]).all() and s2[b] == CANARY and (s2[b + 1:] == s[b:]).all()
        assert (e2[:b] == e[:b]).all() and e2[b] == CANARY and (e2[b + 1:] == e[b:]).all()
        assert (ed2[:2 * b] == ed[:2 * b]).all() and (ed2[2 * b:2 * b + 2] == CANARY).all()
        # total_intervals too small: the slots at and above it are never written
        cut = a + 1
        rc, s2, e2, ed2 = abi_pass2(gi, flat, off, ooff, cut, K=K, cap=total)
        assert rc == L.ERR_ARG
        assert (s2[:cut] == s[:cut]).all() and (s2[cut:] == CANARY).all()
        assert (e2[:cut] == e[:cut]).all() and (e2[cut:] == CANARY).all()
        assert (ed2[:2 * cut] == ed[:2 * cut]).all() and (ed2[2 * cut:] == CANARY).all()
        # offsets that go backwards at one pattern (it has no slot; the next one starts a slot early)
        back = ooff.copy()
        back[kb + 1] = ooff[kb] - np.uint64(1)
        rc, s2, e2, ed2 = abi_pass2(gi, flat, off, back, total, K=K)
        assert rc == L.ERR_ARG and (s2[:a - 1] == s[:a - 1]).all()
        gi.close()


def test_errors():
    n = 20001
    t = dna(n, 95)
    tx = F.Text.with_max_character(t, 4)
    gi = F.FMIndexWithLocate(tx, 2)
    pats, first_hi = make_batch(t, 4, np.random.default_rng(1), per=30, mmax=24)
    assert first_hi is not None
    flat, off = pack(pats, np.uint8)
    npat = len(pats)
    rc, nint, count = abi_pass1(gi, flat, off, K=1)
    assert rc == L.OK                                               # a symbol above max_character is no error
    want = expect_mismatch(O.OracleIndex(t, 4), flat, off, max_mismatches=1)
    assert (nint == want[0]).all() and (count == want[1]).all()
    rc, only_n, none = abi_pass1(gi, flat, off, K=1, want=(True, False))
    assert rc == L.OK and none is None and (only_n == nint).all()
    rc, none, only_c = abi_pass1(gi, flat, off, K=1, want=(False, True))
    assert rc == L.OK and none is None and (only_c == count).all()
    ooff = scan(nint)
    # decreasing offsets: FMX_ERR_ARG, the pattern has no interval, the others keep theirs
    boff = off.copy()
    kb = int(np.nonzero(off >= 1)[0][0])
    boff[kb + 1] = off[kb] - np.uint64(1)
    rc, n2, c2 = abi_pass1(gi, flat, boff, K=1)
    assert rc == L.ERR_ARG and n2[kb] == 0 and c2[kb] == 0
    assert (n2[:kb] == nint[:kb]).all() and (n2[kb + 2:] == nint[kb + 2:]).all()
    # an s0e0 entry above len()
    se = np.tile(np.array([0, n], dtype=np.uint64), npat)
    se[5] = n + 1
    rc, n2, c2 = abi_pass1(gi, flat, off, s0e0=se, K=1)
    assert rc == L.ERR_ARG and n2[2] == 0 and c2[2] == 0
    keep = np.arange(npat) != 2
    assert (n2[keep] == nint[keep]).all() and (c2[keep] == count[keep]).all()
    # a start pair with e <= s emits nothing and is no error
    se = np.tile(np.array([0, n], dtype=np.uint64), npat)
    se[0:4] = [7, 7, 9, 3]
    rc, n2, c2 = abi_pass1(gi, flat, off, s0e0=se, K=1)
    assert rc == L.OK and not n2[:2].any() and not c2[:2].any() and (n2[2:] == nint[2:]).all()
    # max_mismatches = 3: refused before anything is launched, outputs untouched
    rc, n2, c2 = abi_pass1(gi, flat, off, K=3)
    assert rc == L.ERR_ARG and (n2 == 0xDEAD).all() and (c2 == 0xDEAD).all()
    rc, s2, e2, ed2 = abi_pass2(gi, flat, off, ooff, int(ooff[-1]), K=3)
    assert rc == L.ERR_ARG and (s2 == CANARY).all() and (ed2 == CANARY).all()
    gi.close()
    # a handle of the wide engine: FMX_ERR_UNSUPPORTED with a message, outputs untouched
    gw = F.FMIndexWithLocate(tx, 2, force_wide=True)
    assert gw.is_wide()
    rc, n2, c2 = abi_pass1(gw, flat, off, K=1)
    assert rc == L.ERR_UNSUPPORTED and (n2 == 0xDEAD).all() and (c2 == 0xDEAD).all()
    assert b"64-bit" in gw._lib.fmx_last_error()
    rc, s2, e2, ed2 = abi_pass2(gw, flat, off, ooff, int(ooff[-1]), K=1)
    assert rc == L.ERR_UNSUPPORTED and (s2 == CANARY).all() and (e2 == CANARY).all() and (ed2 == CANARY).all()
    gw.close()


def test_empty_text_and_empty_pattern():
    gi = F.FMIndex(F.Text(b""))
    flat, off = pack([np.array(p, dtype=np.uint8) for p in ([1], [], [1, 2], [0])], np.uint8)
    for K in (0, 1, 2):
        rc, nint, count = abi_pass1(gi, flat, off, K=K)
        assert rc == L.OK and not nint.any() and not count.any()
        rc, s, e, ed = abi_pass2(gi, flat, off, np.zeros(5, dtype=np.uint64), 0, K=K, cap=1)
        assert rc == L.OK and s[0] == CANARY
    gi.close()
    t = dna(1000, 5)
    gi = F.FMIndexWithLocate(F.Text.with_max_character(t, 4), 2)
    flat, off = pack([np.zeros(0, dtype=np.uint8)], np.uint8)
    nint, count, s, e, ed = search(gi, flat, off, K=2)                # an empty pattern emits the start pair
    assert nint.tolist() == [1] and count.tolist() == [1000] and (int(s[0]), int(e[0])) == (0, 1000)
    assert (ed == UNUSED).all()
    gi.close()


def test_dev_form_on_a_stream():
    """both passes and fmx_offsets_dev on a non-default stream with torch tensors; the status through
    fmx_stream_status()"""
    import torch
    n = 20001
    t = dna(n, 77)
    gi = F.FMIndexWithLocate(F.Text.with_max_character(t, 4), 2)
    pats, _ = make_batch(t, 4, np.random.default_rng(3), per=40, mmax=24)
    flat, off = pack(pats, np.uint8)
    npat = len(pats)
    K = 2
    wn, wc, ws, we, wed = expect_mismatch(O.OracleIndex(t, 4), flat, off, max_mismatches=K)
    lib = gi._lib
    st = torch.cuda.Stream()

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.int64) if a.dtype == np.uint64 else a).cuda()

    def host(x):
        return x.cpu().numpy().view(np.uint64)

    d_flat, d_off = dev(flat), dev(off)
    d_n = torch.zeros(npat, dtype=torch.int64, device="cuda")
    d_c = torch.zeros(npat, dtype=torch.int64, device="cuda")
    d_zero = torch.zeros(npat, dtype=torch.int64, device="cuda")
    d_oo = torch.zeros(npat + 1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    h = gi.handle()
    assert lib.fmx_mismatch_count_batch_dev(h, d_flat.data_ptr(), d_off.data_ptr(), npat, None, K, d_n.data_ptr(),
                                            d_c.data_ptr(), st.cuda_stream) == L.OK
    assert lib.fmx_offsets_dev(h, d_zero.data_ptr(), d_n.data_ptr(), npat, d_oo.data_ptr(), st.cuda_stream) == L.OK
    st.synchronize()
    assert lib.fmx_stream_status(h) == L.OK
    assert (host(d_n) == wn).all() and (host(d_c) == wc).all() and (host(d_oo) == scan(wn)).all()
    total = int(host(d_oo)[-1])
    d_s = torch.zeros(total, dtype=torch.int64, device="cuda")
    d_e = torch.zeros(total, dtype=torch.int64, device="cuda")
    d_ed = torch.zeros(2 * total, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    assert lib.fmx_mismatch_search_batch_dev(h, d_flat.data_ptr(), d_off.data_ptr(), npat, None, K, d_oo.data_ptr(),
                                             total, d_s.data_ptr(), d_e.data_ptr(), d_ed.data_ptr(),
                                             st.cuda_stream) == L.OK
    st.synchronize()
    assert lib.fmx_stream_status(h) == L.OK
    assert (host(d_s) == ws).all() and (host(d_e) == we).all() and (host(d_ed) == wed).all()
    # a total_intervals that is too small is reported through the status word
    assert lib.fmx_mismatch_search_batch_dev(h, d_flat.data_ptr(), d_off.data_ptr(), npat, None, K, d_oo.data_ptr(),
                                             total - 1, d_s.data_ptr(), d_e.data_ptr(), None, st.cuda_stream) == L.OK
    st.synchronize()
    assert lib.fmx_stream_status(h) == L.ERR_ARG
    assert lib.fmx_stream_status(h) == L.OK                           # reading cleared it
    gi.close()


def test_more_patterns_than_groups():
    """a batch in which every group takes more than one pattern (n = 2^16), against fmx_count_batch at K = 0 and the
    oracle's enumeration on a slice at K = 1"""
    n = 1 << 16
    t = dna(n, 61)
    gi = F.FMIndexWithLocate(F.Text.with_max_character(t, 4), 2)
    npat, m = 150000, 12
    rng = np.random.default_rng(12)
    a = rng.integers(0, n - 1 - m, npat)
    mat = t[a[:, None] + np.arange(m)[None, :]].copy()
    hit = rng.integers(0, 3, npat) > 0
    mat[np.nonzero(hit)[0], rng.integers(0, m, int(hit.sum()))] = rng.integers(1, 5, int(hit.sum()))
    flat = np.ascontiguousarray(mat.reshape(-1))
    off = np.arange(npat + 1, dtype=np.uint64) * np.uint64(m)
    rc, nint, count = abi_pass1(gi, flat, off, K=0)
    rc2, _, _, cc = abi_count(gi, flat, off)
    assert rc == L.OK and rc2 == L.OK and (count == cc).all() and (nint == (cc > 0)).all()
    nint, count, s, e, ed = search(gi, flat, off, K=1)
    assert (count >= cc).all() and int(nint.sum()) == len(s)
    part = slice(npat - 300, npat)
    wn, wc, ws, we, wed = expect_mismatch(O.OracleIndex(t, 4), flat, off[npat - 300:], max_mismatches=1)
    assert (nint[part] == wn).all() and (count[part] == wc).all()
    lo = int(scan(nint)[npat - 300])
    assert (s[lo:] == ws).all() and (e[lo:] == we).all() and (ed[2 * lo:] == wed).all()
    gi.close()


def test_python_mississippi():
    """by hand; the rows of `mississippi$` are  0 $  1 i$  2 ippi$  3 issippi$  4 ississippi$  5 mississippi$  6 pi$
    7 ppi$  8 sippi$  9 sissippi$  10 ssippi$  11 ssissippi$"""
    index = F.FMIndexWithLocate(F.Text(b"mississippi\x00"), 2)
    b = index.mismatch_search_many([b"sip", b"issi", b"m", b""], max_mismatches=1)
    # `sip`: substitutions at pos 2 come first (sym `s`: "sis" at 3), then the exact match ("sip" at 6)
    # `issi`: no neighbour at distance 1 occurs; the exact match at 1 and 4 comes last (and alone)
    # `m`: every other symbol of the text, ascending -- i (4 rows), p (2), s (4) -- then m itself; 0 is never put in
    assert b.nint.tolist() == [2, 1, 4, 1] and b.counts.tolist() == [2, 2, 11, 12]
    assert b.off.tolist() == [0, 2, 3, 7, 8]
    assert list(zip(b.s.tolist(), b.e.tolist())) == [(9, 10), (8, 9), (3, 5), (1, 5), (6, 8), (8, 12), (5, 6), (0, 12)]
    ed = b.edits
    assert ed.shape == (8, 2) and bool(ed.mask[1]["pos"].all()) and not bool(ed.mask[0, 0]["pos"])
    assert (int(ed[0, 0]["pos"]), int(ed[0, 0]["sym"])) == (2, ord("s"))
    assert [(int(ed[j, 0]["pos"]), chr(int(ed[j, 0]["sym"]))) for j in (3, 4, 5)] == [(0, "i"), (0, "p"), (0, "s")]
    hoff, pos = b.locate()
    per_interval = [sorted(pos[int(hoff[j]):int(hoff[j + 1])].tolist()) for j in range(8)]
    assert per_interval[:3] == [[3], [6], [1, 4]]
    assert per_interval[3:7] == [[1, 4, 7, 10], [8, 9], [2, 3, 5, 6], [0]]
    index.close()
