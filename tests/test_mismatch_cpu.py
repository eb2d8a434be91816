"""The checker of the mismatch-search tests is itself checked: tests/mismatch_expect.py (the enumeration of include/fmx.h
over the oracle's lf_map2) against a plain scan of the text on texts of 1 to 300 symbols, and, for patterns that hold a
0, against the oracle's exact search of every enumerated variant.  The last test needs the library but no GPU: the four
entry points refuse a NULL handle before any HIP call."""
import numpy as np
import pytest

from oracle import fm_oracle as O
from mismatch_expect import UNUSED, expect_mismatch, variants


def _windows_within(t, p, K):
    """plain scan: starts of the windows of t within Hamming distance K of p whose mismatching symbols are not 0 (a
    substitution never puts a 0 in), ascending"""
    m = len(p)
    if m > len(t):
        return np.zeros(0, dtype=np.int64)
    if m == 0:
        return np.arange(len(t), dtype=np.int64)
    win = np.lib.stride_tricks.sliding_window_view(t, m).astype(np.int64)
    diff = win != np.asarray(p, dtype=np.int64)[None, :]
    ok = (diff.sum(axis=1) <= K) & ~(diff & (win == 0)).any(axis=1)
    return np.nonzero(ok)[0]


def _order_key(m, eds):
    """the stated order as a sort key: positions from the back of the pattern; a substitution (ascending by symbol)
    comes before the pattern's own symbol"""
    sub = dict(eds)
    return tuple((0, sub[q]) if q in sub else (1, 0) for q in range(m - 1, -1, -1))


def _split(nint, *arrs):
    o = np.concatenate([[0], np.cumsum(nint.astype(np.int64))])
    return [[a[o[k]:o[k + 1]] for a in arrs] for k in range(len(nint))]


def _edits(words):
    return tuple((int(w) >> 32, int(w) & 0xFFFFFFFF) for w in words if w != UNUSED)


def _patterns(t, sigma, rng, per, mmax, with_hi):
    n = len(t)
    pats = []
    for _ in range(per):
        m = int(rng.integers(0, min(mmax, max(n - 1, 0)) + 1))
        a = int(rng.integers(0, max(n - m, 1)))
        p = t[a:a + m].copy()
        p[p == 0] = 1
        pats.append(p)                                              # a substring (the terminator replaced)
        if m:
            q = p.copy()
            q[int(rng.integers(0, m))] = rng.integers(1, sigma + 1)
            pats.append(q)                                          # ... with one symbol changed
            q = q.copy()
            q[int(rng.integers(0, m))] = rng.integers(1, sigma + 1)
            pats.append(q)                                          # ... with two
            if with_hi:
                r = p.copy()
                r[int(rng.integers(0, m))] = sigma + 1 + int(rng.integers(0, 3))
                pats.append(r)                                      # ... with a symbol above max_character
        pats.append(rng.integers(1, sigma + 1, int(rng.integers(0, 5))).astype(np.uint8))
    return pats


@pytest.mark.parametrize("sigma", [4, 20, 200])
@pytest.mark.parametrize("n", [1, 2, 3, 17, 300])
def test_against_a_plain_scan(sigma, n):
    rng = np.random.default_rng(100 * sigma + n)
    t = rng.integers(1, sigma + 1, n).astype(np.uint8)
    t[-1] = 0
    oi = O.OracleIndex(t, sigma, level=1)
    pats = _patterns(t, sigma, rng, 25 if n > 3 else 6, 9, True)
    flat, off = O.pack_patterns([bytes(p) for p in pats])
    seen = set()
    for K in (0, 1, 2):
        nint, count, s, e, ed = expect_mismatch(oi, flat, off, max_mismatches=K)
        assert len(s) == len(e) == int(nint.sum()) and len(ed) == 2 * len(s)
        for k, (ps, pe, pw) in enumerate(_split(nint, s, e, ed.reshape(-1, 2))):
            p = pats[k]
            want = _windows_within(t, p, K)
            assert int(count[k]) == len(want) == int((pe - ps).sum()), (sigma, n, K, k, p.tolist())
            if len(ps) == 0:
                continue
            assert (pe > ps).all()
            order = np.argsort(ps)                                  # pairwise disjoint
            assert (pe[order][:-1] <= ps[order][1:]).all(), (sigma, n, K, k)
            _, pos = oi.locate_batch(ps, pe)
            assert (np.sort(pos.astype(np.int64)) == want).all(), (sigma, n, K, k, p.tolist())
            keys = []
            for j in range(len(ps)):
                eds = _edits(pw[j])
                assert len(eds) <= K and all(b > a for (b, _), (a, _) in zip(eds, eds[1:]))   # nearer the end first
                v = p.copy()
                for q, c in eds:
                    assert 1 <= c <= sigma and c != int(p[q])
                    v[q] = c
                assert (int(ps[j]), int(pe[j])) == oi.search(bytes(v))                       # the variant's own interval
                keys.append(_order_key(len(p), eds))
                seen.add(len(eds))
            assert keys == sorted(keys) and len(set(keys)) == len(keys), (sigma, n, K, k)    # the stated order
    if n == 300:
        assert seen == {0, 1, 2}


@pytest.mark.parametrize("kind", ["fm", "multi"])
def test_patterns_with_a_zero_against_the_exact_search_of_every_variant(kind):
    """a 0 in the pattern is an ordinary symbol and is never substituted IN: the non-empty exact searches of the
    enumerated variants, in order (on a multi-pieces index lf_map2(0, .) is not monotone: e' < s' holds no row)"""
    sigma, n = 4, 300
    rng = np.random.default_rng(7)
    t = rng.integers(1, sigma + 1, n).astype(np.uint8)
    if kind == "multi":
        t[23::41] = 0
    t[-1] = 0
    oi = O.OracleIndex(t, sigma, kind=kind)
    pats = []
    for _ in range(40):
        m = int(rng.integers(1, 8))
        a = int(rng.integers(0, n - m))
        p = t[a:a + m].copy()
        if rng.integers(0, 2):
            p[int(rng.integers(0, m))] = 0
        if rng.integers(0, 3) == 0:
            p[int(rng.integers(0, m))] = rng.integers(1, sigma + 1)
        pats.append(p)
    flat, off = O.pack_patterns([bytes(p) for p in pats])
    some = 0
    for K in (0, 1, 2):
        nint, count, s, e, ed = expect_mismatch(oi, flat, off, max_mismatches=K)
        for k, (ps, pe, pw) in enumerate(_split(nint, s, e, ed.reshape(-1, 2))):
            vs = variants(pats[k], sigma, K)
            vf, vo = O.pack_patterns([bytes(v) for v, _ in vs])
            ws, we = oi.count_batch(vf, vo)
            hit = np.nonzero(we > ws)[0]
            assert (ps == ws[hit]).all() and (pe == we[hit]).all(), (kind, K, k, pats[k].tolist())
            assert [_edits(w) for w in pw] == [vs[j][1] for j in hit]
            some += int((pats[k] == 0).any() and len(hit) > 0)
    assert some >= 10


def test_variants_count_and_order():
    vs = variants(np.array([1, 2, 3], dtype=np.uint8), 4, 1)
    assert len(vs) == 1 + 3 * 3
    assert [v.tolist() for v, _ in vs[:4]] == [[1, 2, 1], [1, 2, 2], [1, 2, 4], [1, 1, 3]]
    assert vs[-1][0].tolist() == [1, 2, 3] and vs[-1][1] == ()
    assert vs[0][1] == ((2, 1),)
    assert len(variants(np.arange(1, 33, dtype=np.uint8) % 4 + 1, 4, 1)) == 97
    assert [v.tolist() for v, _ in variants(np.array([1, 9], dtype=np.uint8), 4, 1)] == [[1, c] for c in (1, 2, 3, 4)]
    assert variants(np.array([1, 9], dtype=np.uint8), 4, 0) == []


def test_entry_points_are_declared_bound_and_exported():
    """the four calls exist in include/fmx.h, in the ctypes table and in libfmx.so, and refuse a NULL handle before
    anything touches a device"""
    import ctypes as C
    import os
    from fm_index_amd import _lib
    names = ["fmx_mismatch_count_batch_dev", "fmx_mismatch_count_batch", "fmx_mismatch_search_batch_dev",
             "fmx_mismatch_search_batch"]
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "fmx.h")).read()
    assert "#define FMX_MAX_MISMATCHES 2" in header
    bound = {s[0]: s for s in _lib.SYMBOLS}
    for nm in names:
        assert "int %s(" % nm in header and nm in bound
    assert [len(bound[nm][2]) for nm in names] == [9, 8, 12, 11]
    lib = _lib.lib()
    off = np.zeros(2, dtype=np.uint64)
    po = off.ctypes.data_as(C.c_void_p)
    assert lib.fmx_mismatch_count_batch(None, None, po, 1, None, 1, None, None) == _lib.ERR_ARG
    assert lib.fmx_mismatch_count_batch_dev(None, None, po, 1, None, 1, None, None, None) == _lib.ERR_ARG
    assert lib.fmx_mismatch_search_batch(None, None, po, 1, None, 1, po, 0, None, None, None) == _lib.ERR_ARG
    assert lib.fmx_mismatch_search_batch_dev(None, None, po, 1, None, 1, po, 0, None, None, None, None) == _lib.ERR_ARG
