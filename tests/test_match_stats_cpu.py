"""The checker of the matching-statistics tests is itself checked: tests/match_stats_expect.py (the loop of include/fmx.h
over the oracle's lf_map2, and the seed rule) against hand-worked answers on `mississippi` and against plain scans of
the text on random texts; and the two entry points exist.  No GPU."""
import numpy as np
import pytest

from oracle import fm_oracle as O
from match_stats_expect import expect_match_stats, seeds_of


def _pack(pats, dtype=np.uint8):
    off = np.zeros(len(pats) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(p) for p in pats], dtype=np.uint64)
    flat = np.concatenate([np.asarray(p, dtype=dtype) for p in pats] + [np.zeros(1, dtype=dtype)])
    return flat, off


def test_mississippi_by_hand():
    """s, si, sis, sisp, sispi: "sis" occurs, "sisp" does not ("p" does), "pi" does, "spi" does not"""
    oi = O.OracleIndex(b"mississippi\x00", 255)
    flat, off = O.pack_patterns([b"sispi"])
    ln, s, e = expect_match_stats(oi, flat, off)
    assert ln.tolist() == [1, 2, 3, 1, 2]
    assert [(int(a), int(b)) for a, b in zip(s, e)] == [oi.search(p) for p in (b"s", b"si", b"sis", b"p", b"pi")]
    ln, s, e = expect_match_stats(oi, flat, off, min_seed_len=1)
    assert ln.tolist() == [1, 2, 3, 1, 2]                                      # the raw statistic either way
    assert [q[:3] for q in seeds_of(off, ln, s, e)] == [(0, 0, 3), (0, 3, 2)]  # "sis" and "pi"
    assert seeds_of(off, ln, s, e)[0][3:] == oi.search(b"sis") and seeds_of(off, ln, s, e)[1][3:] == oi.search(b"pi")
    assert (s[[0, 1, 3]] == 0).all() and (e[[0, 1, 3]] == 0).all()
    ln, s, e = expect_match_stats(oi, flat, off, min_seed_len=3)
    assert [q[:3] for q in seeds_of(off, ln, s, e)] == [(0, 0, 3)]
    ln, s, e = expect_match_stats(oi, flat, off, max_len=2)
    assert ln.tolist() == [1, 2, 2, 1, 2]
    assert (int(s[2]), int(e[2])) == oi.search(b"is")
    ln, s, e = expect_match_stats(oi, flat, off, min_count=0)                  # 0 is treated as 1
    assert ln.tolist() == [1, 2, 3, 1, 2]
    ln, s, e = expect_match_stats(oi, flat, off, min_count=3)                  # "s" and "i" four times, "si" twice
    assert ln.tolist() == [1, 1, 1, 0, 1] and (int(s[3]), int(e[3])) == (0, 0)


def test_batch_slots_and_empty_patterns():
    oi = O.OracleIndex(b"mississippi\x00", 255)
    flat, off = O.pack_patterns([b"ssi", b"", b"x", b"sispi", b""])
    ln, s, e = expect_match_stats(oi, flat, off, min_seed_len=2)
    assert ln.tolist() == [1, 2, 3, 0, 1, 2, 3, 1, 2]
    assert [q[:3] for q in seeds_of(off, ln, s, e)] == [(0, 0, 3), (3, 0, 3), (3, 3, 2)]
    sub = off[3:].copy()                                                       # a slice keeps its absolute offsets
    ln2, s2, e2 = expect_match_stats(oi, flat, sub, min_seed_len=2)
    assert (ln2 == ln[4:]).all() and (s2 == s[4:]).all() and (e2 == e[4:]).all()
    ln, s, e = expect_match_stats(oi, *O.pack_patterns([]))
    assert len(ln) == 0 and len(s) == 0 and len(e) == 0


def test_entry_points_are_declared_bound_and_exported():
    """the two calls exist in include/fmx.h, in the ctypes table and in libfmx.so, and refuse a NULL handle before
    anything touches a device"""
    import ctypes as C
    import os
    from fm_index_amd import _lib
    names = ["fmx_match_stats_batch_dev", "fmx_match_stats_batch"]
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "fmx.h")).read()
    bound = {s[0]: s for s in _lib.SYMBOLS}
    for nm in names:
        assert "int %s(" % nm in header and nm in bound
    assert len(bound["fmx_match_stats_batch_dev"][2]) == 12 and len(bound["fmx_match_stats_batch"][2]) == 10
    lib = _lib.lib()
    off = np.zeros(2, dtype=np.uint64)
    out = np.zeros(1, dtype=np.uint64)
    po, pl = off.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
    assert lib.fmx_match_stats_batch(None, None, po, 1, 1, 0, 0, None, None, pl) == _lib.ERR_ARG
    assert lib.fmx_match_stats_batch_dev(None, None, po, 1, 0, 1, 0, 0, None, None, pl, None) == _lib.ERR_ARG


def _occurrences(t, p):
    """plain scan: number of positions where p occurs in t"""
    if len(p) > len(t):
        return 0
    win = np.lib.stride_tricks.sliding_window_view(t, len(p))
    return int((win == p).all(axis=1).sum())


def _patterns(t, sigma, rng, dt):
    n = len(t)
    pats = []
    for _ in range(12):
        m = int(rng.integers(0, 13))
        if m <= n - 1:
            a = int(rng.integers(0, n - m))
            p = t[a:a + m].copy()                               # a substring
        else:
            p = rng.integers(1, sigma + 1, m).astype(dt)
        pats.append(p)
        if m:
            q = p.copy()                                        # ... with one symbol changed
            q[int(rng.integers(0, m))] = rng.integers(1, sigma + 1)
            pats.append(q)
            q = q.copy()                                        # ... with two
            q[int(rng.integers(0, m))] = rng.integers(1, sigma + 1)
            pats.append(q)
            r = p.copy()                                        # ... with a symbol above max_character
            r[int(rng.integers(0, m))] = sigma + 1 + int(rng.integers(0, 3))
            pats.append(r)
        pats.append(rng.integers(1, sigma + 1, m).astype(dt))   # random
    return pats


@pytest.mark.parametrize("n", [1, 2, 3, 17, 300])
@pytest.mark.parametrize("sigma", [4, 20, 200])
def test_random_texts_against_plain_scans(sigma, n):
    """L[i] is the longest suffix of P[0..i) with >= min_count windows in the text; the interval holds that many rows;
    the kept seeds are exactly the matches not contained in another (brute force over all substrings)"""
    rng = np.random.default_rng(1000 * sigma + n)
    t = rng.integers(1, sigma + 1, n).astype(np.uint8)
    t[-1] = 0
    oi = O.OracleIndex(t, sigma)
    pats = _patterns(t, sigma, rng, np.uint8)
    flat, off = _pack(pats)
    for mc in (1, 2, 3):
        ln, s, e = expect_match_stats(oi, flat, off, min_count=mc)
        ln1, s1, e1 = expect_match_stats(oi, flat, off, min_count=mc, min_seed_len=1)
        ln2, s2, e2 = expect_match_stats(oi, flat, off, min_count=mc, max_len=2)
        assert (ln1 == ln).all() and (ln2 == np.minimum(ln, np.uint64(2))).all()
        kept = set(q[:3] for q in seeds_of(off, ln1, s1, e1))
        for k, p in enumerate(pats):
            m, base = len(p), int(off[k])
            occ = {}                                            # (a, b) -> windows of p[a:b] in the text, b > a
            for a in range(m):
                for b in range(a + 1, m + 1):
                    occ[(a, b)] = _occurrences(t, p[a:b]) if int(p[a:b].max()) <= sigma else 0
            for i in range(1, m + 1):
                want = max([i - a for a in range(i) if occ[(a, i)] >= mc] + [0])
                assert int(ln[base + i - 1]) == want, (sigma, n, mc, k, i, p.tolist())
                rows = int(e[base + i - 1]) - int(s[base + i - 1])
                assert rows == (occ[(i - want, i)] if want else 0), (sigma, n, mc, k, i)
                if want:
                    assert (int(s[base + i - 1]), int(e[base + i - 1])) == oi.search(bytes(p[i - want:i]))
            ok = [ab for ab, o in occ.items() if o >= mc]
            maximal = set((k, a, b - a) for a, b in ok
                          if not any((c <= a and b <= d) and (c, d) != (a, b) for c, d in ok))
            assert set(q for q in kept if q[0] == k) == maximal, (sigma, n, mc, k, p.tolist())
