"""The checker of the longest-suffix-match tests is itself checked: tests/suffix_match_expect.py (the loop of
include/fmx.h over the oracle's lf_map2) against hand-worked answers on `mississippi` and against a plain scan of
the text on random texts.  No GPU."""
import numpy as np
import pytest

from oracle import fm_oracle as O
from suffix_match_expect import expect_suffix_match


def _one(oi, pattern, **kw):
    flat, off = O.pack_patterns([pattern])
    s, e, c, ln = expect_suffix_match(oi, flat, off, **kw)
    return int(s[0]), int(e[0]), int(c[0]), int(ln[0])


def test_mississippi_by_hand():
    oi = O.OracleIndex(b"mississippi\x00", 255)
    assert _one(oi, b"pssi") == (10, 12, 2, 3)              # "ssi" occurs twice, "pssi" never
    assert _one(oi, b"pssi", min_count=3) == (1, 5, 4, 1)   # "i" four times, "si" only twice
    assert _one(oi, b"ssi") == (10, 12, 2, 3)
    assert _one(oi, b"x") == (0, 12, 12, 0)
    assert _one(oi, b"") == (0, 12, 12, 0)
    assert _one(oi, b"ssi", min_count=0) == (10, 12, 2, 3)  # 0 is treated as 1


def test_mississippi_refinement_and_batch():
    oi = O.OracleIndex(b"mississippi\x00", 255)
    si = oi.search(b"si")
    assert _one(oi, b"xis", s0e0=[si[0], si[1]]) == oi.search(b"issi") + (2, 2)   # "is" prepended to "si", then "x" fails
    flat, off = O.pack_patterns([b"pssi", b"", b"x", b"ssi"])
    s, e, c, ln = expect_suffix_match(oi, flat, off)
    assert ln.tolist() == [3, 0, 0, 3] and c.tolist() == [2, 12, 12, 2] and s.tolist() == [10, 0, 0, 10]


def test_entry_points_are_declared_bound_and_exported():
    """the three calls exist in include/fmx.h, in the ctypes table and in libfmx.so, and refuse a NULL handle before
    anything touches a device"""
    import ctypes as C
    import os
    from fm_index_amd import _lib
    names = ["fmx_suffix_match_batch_dev", "fmx_suffix_match_batch", "fmx_suffix_match_batch_multi"]
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "fmx.h")).read()
    bound = {s[0]: s for s in _lib.SYMBOLS}
    for nm in names:
        assert "int %s(" % nm in header and nm in bound
    assert len(bound["fmx_suffix_match_batch_dev"][2]) == 11 and len(bound["fmx_suffix_match_batch"][2]) == 10
    assert len(bound["fmx_suffix_match_batch_multi"][2]) == 11
    lib = _lib.lib()
    off = np.zeros(2, dtype=np.uint64)
    po = off.ctypes.data_as(C.c_void_p)
    assert lib.fmx_suffix_match_batch(None, None, po, 1, None, 1, None, None, None, None) == _lib.ERR_ARG
    assert lib.fmx_suffix_match_batch_dev(None, None, po, 1, None, 1, None, None, None, None, None) == _lib.ERR_ARG
    assert lib.fmx_suffix_match_batch_multi(None, 0, None, po, 1, None, 1, None, None, None, None) == _lib.ERR_ARG
    hs = (C.c_void_p * 2)(None, None)
    assert lib.fmx_suffix_match_batch_multi(hs, 2, None, po, 1, None, 1, None, None, None, None) == _lib.ERR_ARG


def _occurrences(t, p):
    """plain scan: number of positions where p occurs in t (numpy; the empty pattern occurs len(t) times, as (0, len))"""
    if len(p) == 0:
        return len(t)
    if len(p) > len(t):
        return 0
    win = np.lib.stride_tricks.sliding_window_view(t, len(p))
    return int((win == p).all(axis=1).sum())


@pytest.mark.parametrize("sigma", [4, 200])
def test_random_texts_against_a_plain_scan(sigma):
    n = 300
    rng = np.random.default_rng(1000 + sigma)
    t = rng.integers(1, sigma + 1, n).astype(np.uint8)
    t[-1] = 0
    oi = O.OracleIndex(t, sigma)
    pats = []
    for _ in range(150):
        m = int(rng.integers(0, 13))
        a = int(rng.integers(0, n - 1 - m))
        p = t[a:a + m].copy()                               # a substring
        pats.append(p)
        if m:
            q = p.copy()                                    # ... with one symbol changed
            q[int(rng.integers(0, m))] = rng.integers(1, sigma + 1)
            pats.append(q)
            r = p.copy()                                    # ... with a symbol above max_character
            r[int(rng.integers(0, m))] = sigma + 1 + int(rng.integers(0, 3))
            pats.append(r)
        pats.append(rng.integers(1, sigma + 1, m).astype(np.uint8))   # random
    flat, off = O.pack_patterns([bytes(p) for p in pats])
    for p in [p for p in pats if len(p)][:20]:              # the scan itself against the oracle's NaiveSearchIndex
        assert _occurrences(t, p) == len(O.naive_search(t, p))
    for mc in (1, 2, 5):
        s, e, c, ln = expect_suffix_match(oi, flat, off, min_count=mc)
        for k, p in enumerate(pats):
            occ = [_occurrences(t, p[len(p) - L:]) for L in range(len(p) + 1)]
            want = max(L for L in range(len(p) + 1) if all(o >= mc for o in occ[:L + 1]))
            assert int(ln[k]) == want, (sigma, mc, k, p.tolist())
            assert int(c[k]) == occ[want] and int(e[k] - s[k]) == occ[want], (sigma, mc, k)
            if want:                                        # the interval is the one search() gives for that suffix
                assert (int(s[k]), int(e[k])) == oi.search(bytes(p[len(p) - want:]))
