"""What the four host-array pattern calls (fmx_count_batch, fmx_suffix_match_batch, fmx_mismatch_count_batch /
fmx_mismatch_search_batch, fmx_match_stats_batch) have in common before anything is launched: the span
pat[pat_off[0] .. pat_off[npat]) they move, Character = u64 symbols narrowed with saturation, and the refusal of offsets
whose last entry lies below the first.  A text of 300 symbols and a few dozen patterns, once as u8 and once as u64."""
import numpy as np
import pytest

import fm_index_amd as F
from fm_index_amd import _lib as L
from oracle import fm_oracle as O
from match_stats_expect import expect_match_stats
from mismatch_expect import expect_mismatch
from suffix_match_expect import expect_suffix_match
from test_gpu_match_stats import abi_ms
from test_gpu_mismatch import abi_pass1, search
from test_gpu_suffix_match import abi_count, abi_match, dna, make_batch, pack

pytestmark = pytest.mark.gpu

N, MAXC = 300, 4
WRAP = np.uint64(1) << np.uint64(32)          # a symbol c + WRAP narrows to c if the upper half is dropped


@pytest.fixture(scope="module", params=[np.uint8, np.uint64], ids=["u8", "u64"])
def index(request):
    t = dna(N, 7).astype(request.param)
    gi = F.FMIndexWithLocate(F.Text.with_max_character(t, MAXC), 2)
    assert gi._dtype == request.param                       # (fmx_build was given sym_bytes = the item size)
    yield gi, t
    gi.close()


@pytest.fixture(scope="module")
def index_u64():
    t = dna(N, 7).astype(np.uint64)
    gi = F.FMIndexWithLocate(F.Text.with_max_character(t, MAXC), 2)
    assert gi._dtype == np.uint64
    yield gi, t
    gi.close()


def valid_batch(t, seed, per=10):
    """substrings, substrings with one symbol changed, random patterns and two empty ones; every symbol in 1 .. MAXC"""
    pats, _ = make_batch(t, MAXC, np.random.default_rng(seed), per=per, mmax=24)
    pats = [p for p in pats if len(p) == 0 or (p.min() >= 1 and p.max() <= MAXC)]
    pats.insert(2, t[:0].copy())
    pats.append(t[:0].copy())
    return pats


def test_u64_symbols_above_2_32_saturate(index_u64):
    """a substring of the text with 2^32 added to one symbol: still out of range after narrowing, so count reports it and
    the other three end the match there -- the oracle gets the same batch with every such symbol as max_character + 1"""
    gi, t = index_u64
    oi = O.OracleIndex(t.astype(np.uint8), MAXC)
    rng = np.random.default_rng(3)
    pats = valid_batch(t, 11, per=6)
    nvalid = len(pats)
    for j in (0, 3, 7):                                   # the last, a middle and the first symbol of an 8-symbol substring
        a = int(rng.integers(0, N - 9))
        p = t[a:a + 8].copy()
        p[7 - j] += WRAP
        pats.append(p)
    p = t[5:13].copy()
    p[4] = np.uint64(0xFFFFFFFFFFFFFFFF)
    pats.append(p)
    flat, off = pack(pats, np.uint64)
    assert int(flat.max()) > int(WRAP)
    seen = np.minimum(flat, np.uint64(MAXC + 1))          # what the index sees: out of range stays out of range
    npat = len(pats)
    m = np.diff(off.astype(np.int64))

    # count: reported for the batch and for every such pattern alone; the valid patterns alone give the oracle's rows
    assert abi_count(gi, flat, off)[0] == L.ERR_SYMBOL_RANGE
    for k in range(nvalid, npat):
        assert abi_count(gi, flat, off[k:k + 2])[0] == L.ERR_SYMBOL_RANGE, k
    ws, we, wc, wl = expect_suffix_match(oi, seen, off)
    rc, s, e, c = abi_count(gi, flat, off[:nvalid + 1])
    assert rc == L.OK, gi._lib.fmx_last_error()
    full = wl[:nvalid] == m[:nvalid].astype(np.uint64)
    assert full.any() and (~full).any()
    assert (c == np.where(full, wc[:nvalid], 0)).all()
    assert (s[full] == ws[:nvalid][full]).all() and (e[full] == we[:nvalid][full]).all()

    # suffix match: no error, the match ends below the symbol (a wrapped symbol would match all eight)
    rc, s, e, c, ln = abi_match(gi, flat, off)
    assert rc == L.OK, gi._lib.fmx_last_error()
    assert (s == ws).all() and (e == we).all() and (c == wc).all() and (ln == wl).all()
    assert ln[nvalid:nvalid + 3].tolist() == [0, 3, 7] and int(ln[npat - 1]) == 3

    # mismatch search, both passes: the symbol has to be one of the substitutions
    for K in (0, 1):
        got = search(gi, flat, off, K=K)
        want = expect_mismatch(oi, seen, off, max_mismatches=K)
        for g, w in zip(got, want):
            assert len(g) == len(w) and (g == w).all(), K
        assert not got[0][nvalid:].any() if K == 0 else got[0][nvalid:].all()

    # matching statistics
    rc, ln, s, e = abi_ms(gi, flat, off)
    assert rc == L.OK, gi._lib.fmx_last_error()
    wl, ws, we = expect_match_stats(oi, seen, off)
    assert (ln == wl).all() and (s == ws).all() and (e == we).all()


def test_slice_of_a_larger_batch(index):
    """entries a .. b of a batch's offsets with the whole pattern buffer (pat_off[0] > 0): the results of those patterns"""
    gi, t = index
    pats = valid_batch(t, 21)
    flat, off = pack(pats, t.dtype)
    npat = len(pats)
    w_count = abi_count(gi, flat, off)
    w_match = abi_match(gi, flat, off, min_count=2)
    w_mm = search(gi, flat, off, K=1)
    w_ms = abi_ms(gi, flat, off, 1, 0, 3)
    assert w_count[0] == L.OK and w_match[0] == L.OK and w_ms[0] == L.OK
    istart = np.zeros(npat + 1, dtype=np.int64)
    istart[1:] = np.cumsum(w_mm[0].astype(np.int64))
    for a, b in ((1, npat), (5, 6), (npat // 2, npat - 3), (2, 3)):      # (2, 3): the empty pattern alone, span 0
        sl = off[a:b + 1]
        assert int(sl[0]) > 0
        lo, hi = int(off[a]), int(off[b])
        got = abi_count(gi, flat, sl)
        assert got[0] == L.OK, gi._lib.fmx_last_error()
        for g, w in zip(got[1:], w_count[1:]):
            assert (g == w[a:b]).all(), (a, b)
        got = abi_match(gi, flat, sl, min_count=2)
        assert got[0] == L.OK
        for g, w in zip(got[1:], w_match[1:]):
            assert (g == w[a:b]).all(), (a, b)
        got = search(gi, flat, sl, K=1)
        assert (got[0] == w_mm[0][a:b]).all() and (got[1] == w_mm[1][a:b]).all()
        ia, ib = int(istart[a]), int(istart[b])
        assert (got[2] == w_mm[2][ia:ib]).all() and (got[3] == w_mm[3][ia:ib]).all()
        assert (got[4] == w_mm[4][2 * ia:2 * ib]).all()
        got = abi_ms(gi, flat, sl, 1, 0, 3)
        assert got[0] == L.OK
        for g, w in zip(got[1:], w_ms[1:]):
            assert len(g) == hi - lo and (g == w[lo:hi]).all(), (a, b)


def test_slice_whose_last_offset_lies_below_its_first(index):
    gi, t = index
    pats = valid_batch(t, 21)
    flat, off = pack(pats, t.dtype)
    a, b = 5, len(pats) - 3
    sl = off[a:b + 1].copy()
    sl[-1] = sl[0] - np.uint64(1)
    assert abi_count(gi, flat, sl)[0] == L.ERR_ARG
    assert abi_match(gi, flat, sl)[0] == L.ERR_ARG
    assert abi_pass1(gi, flat, sl)[0] == L.ERR_ARG
    assert abi_ms(gi, flat, sl)[0] == L.ERR_ARG
    assert abi_count(gi, flat, off[a:b + 1])[0] == L.OK                 # and the handle still works afterwards
