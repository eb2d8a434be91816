"""The one-pass mismatch search on 2-bit packed DNA patterns, one strand or both (fmx_mismatch_hits_batch_packed2* /
mismatch_hits_many_packed*), against the enumeration of include/fmx.h run over the CPU oracle (tests/mismatch_expect.py)
on the bytes of each strand -- the reverse complement built here by plain numpy -- cut to the first max_hits intervals."""
import ctypes as C

import numpy as np
import pytest

import fm_index_amd as F
from fm_index_amd import _lib as L
from fm_index_amd import workload as W
from oracle import fm_oracle as O
from mismatch_expect import UNUSED, expect_mismatch

pytestmark = pytest.mark.gpu

VARIANTS = {"plain": dict(plain=True), "pair-kmer": dict(pair_index=True, kmer_table=True)}
CANARY = np.uint64(0xC0FFEE)
EXPECT = {}                                                         # (n, K, strands) -> the batch and the oracle's answer


def call(gi, words, off, K, max_hits, strands=1, skip=()):
    """the C call itself: (code, nint, count, s, e, edit); the arrays named in `skip` are passed as NULL; eight
    canaries behind every array are checked here"""
    nv = strands * (len(off) - 1)
    sizes = dict(nint=nv, count=nv, s=nv * max_hits, e=nv * max_hits, edit=2 * nv * max_hits)
    a = {k: np.full(sz + 8, CANARY, dtype=np.uint64) for k, sz in sizes.items()}
    name = "fmx_mismatch_hits_batch_packed2_rc" if strands == 2 else "fmx_mismatch_hits_batch_packed2"
    rc = getattr(gi._lib, name)(gi.handle(), words.ctypes.data_as(C.c_void_p), off.ctypes.data_as(C.c_void_p),
                                len(off) - 1, K, max_hits,
                                *(None if k in skip else a[k].ctypes.data_as(C.c_void_p) for k in sizes))
    for k, sz in sizes.items():
        assert (a[k][sz:] == CANARY).all() and (k not in skip or (a[k] == CANARY).all()), k
    return (rc,) + tuple(a[k][:sz] for k, sz in sizes.items())


def revcomp(flat, off):
    r = flat.copy()
    for a, b in zip(off[:-1].astype(np.int64), off[1:].astype(np.int64)):
        r[a:b] = 5 - flat[a:b][::-1]
    return r


@pytest.mark.parametrize("strands", [1, 2])
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("K", [0, 1, 2])
@pytest.mark.parametrize("n", [4, 9, 130, 1000])
def test_first_hits_of_every_strand_equal_the_oracle(n, K, variant, strands):
    """ragged random patterns (empty, length 1, odd, even) and text substrings of 31, 32, 33, 64 and 65 symbols with
    every 17th symbol changed (on two strands also their reverse complements, so the odd entries match): frames resume
    on either side of every refill.  The kinds of entry every case with n >= 130 must hold are asserted from the
    oracle alone; `nint > max_hits` cannot exist for K = 0 (an exact search emits at most one interval) and is asked
    for K >= 1 only."""
    if (n, K, strands) not in EXPECT:
        t = W.dna_text_np(n, 500 + n)
        oi = O.OracleIndex(t, 4)
        flat, off = W.ragged_patterns_np(150, 40, 4, 510 + n)
        parts, lens = [flat[:int(off[-1])]], list(np.diff(off.astype(np.int64)))
        for m in (31, 32, 33, 64, 65) if n >= 130 else ():
            sf, so, _ = W.substring_patterns_np(t, 6, m, 520 + n + m)
            q = np.arange(16, len(sf), 17)
            sf[q] = sf[q] % 4 + 1
            parts += [sf] + ([revcomp(sf, so)] if strands == 2 else [])
            lens += [m] * (6 * strands)
        flat = np.concatenate(parts)
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
        want = [expect_mismatch(oi, f, off, None, K) for f in ((flat, revcomp(flat, off))[:strands])]
        EXPECT[(n, K, strands)] = (t, flat, off, want)
    t, flat, off, want = EXPECT[(n, K, strands)]
    npat = len(off) - 1
    gi = F.FMIndex(F.Text.with_max_character(t, 4), **VARIANTS[variant])
    words, _ = F.pack2(flat=flat, off=off)
    for max_hits in (1, 3):
        rc, nint, cnt, s, e, ed = call(gi, words, off, K, max_hits, strands)
        assert rc == L.OK, gi._lib.fmx_last_error()
        kinds = set()
        for strand, (wn, wc, ws, we, wed) in enumerate(want):
            first = np.concatenate([[0], np.cumsum(wn)]).astype(np.int64)
            for k in range(npat):
                v, have = strands * k + strand, min(int(wn[k]), max_hits)
                kinds.add("over" if wn[k] > max_hits else "fits" if wn[k] else "none")
                assert nint[v] == wn[k] and cnt[v] == wc[k], (v, max_hits)
                a, b = v * max_hits, first[k]
                assert (s[a:a + have] == ws[b:b + have]).all() and (e[a:a + have] == we[b:b + have]).all(), v
                assert (ed[2 * a:2 * (a + have)] == wed[2 * b:2 * (b + have)]).all(), v
                assert not s[a + have:a + max_hits].any() and not e[a + have:a + max_hits].any(), v
                assert (ed[2 * (a + have):2 * (a + max_hits)] == UNUSED).all(), v
        if n >= 130:
            assert kinds == ({"over", "fits", "none"} if K else {"fits", "none"}), (kinds, max_hits)
    gi.close()


def test_every_alignment_slice_and_foreign_bits():
    """a pattern starts and one ends at every offset mod 32, one of length 1 sits in the last 2 bits of a word; even
    patterns are text substrings, odd ones reverse complements of text substrings, every 97th symbol is changed; the
    batch as it is and as a slice from symbol 37, the bits that belong to no pattern all 0 and all 1"""
    t = W.dna_text_np(5000, 41)
    gi = F.FMIndex(F.Text.with_max_character(t, 4), pair_index=True, kmer_table=True)
    oi = O.OracleIndex(t, 4)
    lens = [31, 1] + [33 + k % 3 for k in range(96)] + [0, 1, 2, 64]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    assert int(off[2]) == 32 and int(off[1]) == 31                  # pattern 1: one symbol in the last 2 bits of word 0
    assert {int(o) % 32 for o in off[:-1]} == set(range(32)) and {int(o) % 32 for o in off[1:]} == set(range(32))
    flat = W.substring_patterns_np(t, 1, int(off[-1]), 43)[0]
    other = revcomp(W.substring_patterns_np(t, 1, int(off[-1]), 44)[0], off)
    for k in range(1, len(lens), 2):
        flat[int(off[k]):int(off[k + 1])] = other[int(off[k]):int(off[k + 1])]
    q = np.arange(50, len(flat), 97)
    flat[q] = flat[q] % 4 + 1
    want = [expect_mismatch(oi, f, off, None, 1) for f in (flat, revcomp(flat, off))]
    for strand in (0, 1):                                           # hits and misses on each strand
        assert (want[strand][0] > 0).any() and (want[strand][0] == 0).any()
    got = []
    for lead in (0, 37):
        o = off + np.uint64(lead)
        words, _ = F.pack2(flat=np.concatenate([np.ones(lead, dtype=np.uint8), flat]), off=o)
        unused = np.ones(32 * len(words), dtype=np.uint64)
        unused[int(o[0]):int(o[-1])] = 0
        ones = ((unused * np.uint64(3)).reshape(-1, 32) << (np.arange(32, dtype=np.uint64) * np.uint64(2))).sum(
            axis=1, dtype=np.uint64)
        assert int(o[-1]) % 32 != 0 and (lead == 0 or ones[0] == np.uint64(0xFFFFFFFFFFFFFFFF))
        got += [call(gi, w, o, 1, 2, strands=2) for w in (words, words | ones)]
    for r in got:
        assert r[0] == L.OK and all((x == y).all() for x, y in zip(r[1:], got[0][1:]))
    rc, nint, cnt, s, e, ed = got[0]
    for strand, (wn, wc, ws, we, wed) in enumerate(want):
        assert (nint[strand::2] == wn).all() and (cnt[strand::2] == wc).all()
        first = np.concatenate([[0], np.cumsum(wn)]).astype(np.int64)
        for k in np.nonzero(wn)[0]:                                 # the first interval and its edits
            v = 2 * int(k) + strand
            assert s[2 * v] == ws[first[k]] and e[2 * v] == we[first[k]] and (ed[4 * v:4 * v + 2] == wed[2 * first[k]:2 * first[k] + 2]).all()
    gi.close()


def test_contract():
    import torch
    t = W.dna_text_np(20000, 3)
    gi = F.FMIndexWithLocate(F.Text.with_max_character(t, 4), 2, pair_index=True, kmer_table=True)
    flat, off = W.ragged_patterns_np(300, 14, 4, 5)
    words, _ = F.pack2(flat=flat, off=off)
    npat = len(off) - 1
    ref = call(gi, words, off, 1, 4, strands=2)
    assert ref[0] == L.OK and (ref[1] > 4).any()
    # max_hits = 0: only the totals; NULL arrays are accepted and the others unchanged by it
    rc, nint, cnt, s, e, ed = call(gi, words, off, 1, 0, strands=2)
    assert rc == L.OK and (nint == ref[1]).all() and (cnt == ref[2]).all() and len(s) == len(ed) == 0
    part = call(gi, words, off, 1, 4, strands=2, skip=("nint", "e", "edit"))
    assert part[0] == L.OK and (part[2] == ref[2]).all() and (part[3] == ref[3]).all()
    assert call(gi, words, off, 1, 4, strands=2, skip=("nint", "count", "s", "e", "edit"))[0] == L.OK
    # decreasing offsets: that pattern holds zeros and the filler on both strands, the others are right
    o = off.copy()
    o[8] = o[7] - np.uint64(2)
    rc, nint, cnt, s, e, ed = call(gi, words, o, 1, 4, strands=2)
    assert rc == L.ERR_ARG
    for v in range(2 * npat):
        if v // 2 == 7:
            assert nint[v] == cnt[v] == 0 and not s[4 * v:4 * v + 4].any() and not e[4 * v:4 * v + 4].any()
            assert (ed[8 * v:8 * v + 8] == UNUSED).all()
        elif v // 2 != 8:                                           # (pattern 8 grew by two symbols)
            assert nint[v] == ref[1][v] and cnt[v] == ref[2][v] and (s[4 * v:4 * v + 4] == ref[3][4 * v:4 * v + 4]).all()
            assert (ed[8 * v:8 * v + 8] == ref[5][8 * v:8 * v + 8]).all()
    # max_mismatches above FMX_MAX_MISMATCHES: refused before anything is written
    bad = call(gi, words, off, 3, 4, strands=2)
    assert bad[0] == L.ERR_ARG and all((x == CANARY).all() for x in bad[1:])
    # the dev form on a stream == the host form
    dw, do = torch.from_numpy(words.view(np.int64)).cuda(), torch.from_numpy(off.view(np.int64)).cuda()
    outs = [torch.zeros(max(len(x), 1), dtype=torch.int64, device="cuda") for x in ref[1:]]
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        rc = gi._lib.fmx_mismatch_hits_batch_packed2_rc_dev(gi.handle(), dw.data_ptr(), do.data_ptr(), npat, 1, 4,
                                                            *(x.data_ptr() for x in outs), st.cuda_stream)
    st.synchronize()
    assert rc == L.OK and gi._lib.fmx_stream_status(gi.handle()) == L.OK
    for x, y in zip(outs, ref[1:]):
        assert (x.cpu().numpy().view(np.uint64)[:len(y)] == y).all()
    # the Python surface: the same arrays; .locate() of an untruncated batch == locate_many of the byte call's intervals
    h = gi.mismatch_hits_many_packed_both_strands(words, off, max_mismatches=1, max_hits=4)
    assert (h.nint == ref[1]).all() and (h.counts == ref[2]).all() and (h.s.reshape(-1) == ref[3]).all()
    assert (h.e.reshape(-1) == ref[4]).all() and (h.truncated == (ref[1] > 4)).all()
    assert (h.edits["sym"].mask.reshape(-1) == (ref[5] == UNUSED)).all()
    assert (h.edits["pos"].data.reshape(-1)[ref[5] != UNUSED] == ref[5][ref[5] != UNUSED] >> np.uint64(32)).all()
    h = gi.mismatch_hits_many_packed(words, off, max_mismatches=1, max_hits=int(ref[1].max()))
    mb = gi.mismatch_search_many(flat=flat, off=off, max_mismatches=1)
    assert not h.truncated.any() and (h.nint == mb.nint).all() and (h.counts == mb.counts).all()
    assert (h.locate()[1] == gi.locate_many(mb.s, mb.e)[1]).all() and len(h.locate()[1]) == int(mb.counts.sum())
    gi.close()


@pytest.mark.parametrize("make", [
    lambda t: F.RLFMIndex(F.Text.with_max_character(t, 4)),
    lambda t: F.FMIndex(F.Text.with_max_character(t, 4), force_wide=True),
], ids=["rlfm", "wide"])
def test_other_indexes_are_refused_and_nothing_is_written(make):
    gi = make(W.dna_text_np(3000, 8))
    flat, off = W.ragged_patterns_np(50, 9, 4, 10)
    words, _ = F.pack2(flat=flat, off=off)
    for strands in (1, 2):
        r = call(gi, words, off, 1, 2, strands)
        assert r[0] == L.ERR_UNSUPPORTED and all((x == CANARY).all() for x in r[1:])
    gi.close()


def test_three_symbol_alphabet_single_strand_only():
    """max_character = 3: the both-strand call refuses the handle; the single-strand call serves it and code 3 (symbol
    4, no symbol of the index) costs a substitution where it stands"""
    t = np.minimum(W.dna_text_np(3000, 8), 3)
    gi = F.FMIndex(F.Text.with_max_character(t, 3), plain=True)
    flat, off = W.ragged_patterns_np(200, 9, 4, 10)
    words, _ = F.pack2(flat=flat, off=off)
    r = call(gi, words, off, 1, 2, strands=2)
    assert r[0] == L.ERR_UNSUPPORTED and all((x == CANARY).all() for x in r[1:])
    four = np.array([(flat[int(a):int(b)] == 4).any() for a, b in zip(off[:-1], off[1:])])
    for K in (0, 1, 2):
        wn, wc, ws, we, wed = expect_mismatch(O.OracleIndex(t, 3), flat, off, None, K)
        rc, nint, cnt, s, e, ed = call(gi, words, off, K, 1)
        assert rc == L.OK and (nint == wn).all() and (cnt == wc).all() and (K == 0 or (nint[four] > 0).any())
        first = (np.cumsum(wn) - wn).astype(np.int64)[wn > 0]
        assert (s[wn > 0] == ws[first]).all() and (e[wn > 0] == we[first]).all()
        assert (ed.reshape(-1, 2)[wn > 0] == wed.reshape(-1, 2)[first]).all()
    gi.close()
