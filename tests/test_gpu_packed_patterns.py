"""2-bit packed DNA patterns (fmx_count_batch_packed2 / search_many_packed): the oracle's (s, e) on the UNPACKED bytes,
and the byte call's outputs and error on the same index, for every kernel the packed dispatch can pick."""
import ctypes as C

import numpy as np
import pytest

import fm_index_amd as F
from fm_index_amd import _lib as L
from fm_index_amd import workload as W
from oracle import fm_oracle as O

pytestmark = pytest.mark.gpu

VARIANTS = {"plain": dict(plain=True), "pair": dict(pair_index=True), "pair-kmer": dict(pair_index=True, kmer_table=True),
            "plain-kmer": dict(plain=True, kmer_table=True)}
CANARY = 0xC0FFEE


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def call(gi, name, pat, off, se=None):
    """the C call itself: (code, s, e, count) -- the arrays come back whatever the code is"""
    npat = len(off) - 1
    s, e, c = (np.full(max(npat, 1), CANARY, dtype=np.uint64) for _ in range(3))
    rc = getattr(gi._lib, name)(gi.handle(), _p(pat), _p(off), npat, _p(se), _p(s), _p(e), _p(c))
    return rc, s[:npat], e[:npat], c[:npat]


def agree(gi, oi, flat, off, se=None, words=None):
    """packed call == byte call (code and arrays); with a clean code, == oracle.  Returns the packed (code, s, e)."""
    if words is None:
        words, _ = F.pack2(flat=flat, off=off)
    rp, ps, pe, pc = call(gi, "fmx_count_batch_packed2", words, off, se)
    rb, bs, be, bc = call(gi, "fmx_count_batch", flat, off, se)
    assert rp == rb, (rp, rb, gi._lib.fmx_last_error())
    assert (ps == bs).all() and (pe == be).all() and (pc == bc).all() and (pc == pe - ps).all()
    if rp == L.OK:
        s, e = oi.count_batch(flat, off, se)
        assert (ps == s).all() and (pe == e).all()
    return rp, ps, pe


@pytest.mark.parametrize("n", [4, 9, 130, 1000, 70001])
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_ragged_and_substring_patterns(variant, n):
    t = W.dna_text_np(n, 300 + n)
    gi = F.FMIndex(F.Text.with_max_character(t, 4), **VARIANTS[variant])
    oi = O.OracleIndex(t, 4)
    assert gi.packed2_supported()
    assert gi.has_pair_index() == ("pair" in variant and n >= 4)
    if "kmer" in variant and n >= 1000:
        assert gi.kmer_k() >= 2
    flat, off = W.ragged_patterns_np(3000, 70, 4, 310 + n)          # empty, odd, even; refills at 32 and 64
    assert agree(gi, oi, flat, off)[0] == L.OK
    if n >= 130:
        for m in (31, 32, 33, 64, 65):                              # long matches through every window boundary
            sflat, soff, _ = W.substring_patterns_np(t, 300, m, 320 + n + m)
            rc, s, e = agree(gi, oi, sflat, soff)
            assert rc == L.OK and (e > s).all()
    b = gi.search_many_packed(*F.pack2(flat=flat, off=off))         # the Python surface: the same SearchBatch
    assert (b.s == gi.search_many(flat=flat, off=off).s).all() and (b.counts == b.e - b.s).all()
    gi.close()


@pytest.mark.parametrize("variant", ["plain-kmer", "pair-kmer"])
def test_every_alignment_and_unused_bits(variant):
    """a pattern starts at every offset mod 32 and one ends at every offset mod 32 (lengths 33 + (k mod 3) walk through
    the residues), some end exactly at a word end, one of length 1 sits in the last 2 bits of a word; the bits of the
    words that belong to no pattern of the call are all 0, all 1, and -- for a slice that starts at symbol 37 --
    ones in every word in front of it too"""
    t = W.dna_text_np(5000, 41)
    gi = F.FMIndex(F.Text.with_max_character(t, 4), **VARIANTS[variant])
    oi = O.OracleIndex(t, 4)
    lens = [31, 1] + [33 + k % 3 for k in range(96)] + [0, 1, 2, 64]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    assert int(off[2]) == 32 and int(off[1]) == 31                  # pattern 1: one symbol in the last 2 bits of word 0
    assert {int(o) % 32 for o in off[:-1]} == set(range(32)) and {int(o) % 32 for o in off[1:]} == set(range(32))
    flat = W.substring_patterns_np(t, 1, int(off[-1]), 43)[0]       # matches that run through the window boundaries
    q = np.arange(50, len(flat), 97)
    flat[q] = flat[q] % 4 + 1                                       # ... and some that end early
    ref = agree(gi, oi, flat, off)
    assert ref[0] == L.OK and (ref[2] > ref[1]).any() and (ref[2] == ref[1]).any()
    for lead in (0, 37):                                            # the batch; the same batch as a slice from symbol 37
        o = off + np.uint64(lead)
        f = np.concatenate([np.ones(lead, dtype=np.uint8), flat])
        words, _ = F.pack2(flat=f, off=o)
        unused = np.ones(32 * len(words), dtype=np.uint64)
        unused[int(o[0]):int(o[-1])] = 0
        ones = ((unused * np.uint64(3)).reshape(-1, 32) << (np.arange(32, dtype=np.uint64) * np.uint64(2))).sum(
            axis=1, dtype=np.uint64)
        assert int(o[-1]) % 32 != 0 and (lead == 0 or ones[0] == np.uint64(0xFFFFFFFFFFFFFFFF))
        for w in (words, words | ones):
            rc, s, e = agree(gi, oi, f, o, words=w)
            assert rc == L.OK and (s == ref[1]).all() and (e == ref[2]).all()
    gi.close()


@pytest.mark.parametrize("pair", [False, True])
@pytest.mark.parametrize("maxc", [2, 3])
def test_small_alphabets_refuse_a_code_when_it_is_reached(maxc, pair):
    t = (W.splitmix64_np(5 + maxc, 0, 5000) % np.uint64(maxc)).astype(np.uint8) + 1
    t[-1] = 0
    gi = F.FMIndex(F.Text.with_max_character(t, maxc), pair_index=pair, kmer_table=True, plain=not pair)
    oi = O.OracleIndex(t, maxc)
    assert gi.packed2_supported() and gi.has_pair_index() == pair and gi.kmer_k() >= 2
    good, goff = W.ragged_patterns_np(400, 40, maxc, 11)
    assert agree(gi, oi, good, goff)[0] == L.OK
    pats = []
    for k in range(120):                                            # substrings and random patterns, one code too large
        m = 3 + k % 38
        p = t[k * 7:k * 7 + m].copy() if k % 2 else good[k * 5:k * 5 + m].copy()
        p[[m - 1, m - 2, m // 3][k % 3]] = maxc + 1 + (k % (4 - maxc))
        pats.append(bytes(p))
    flat, off = F.pack_patterns(pats)
    rc, s, e = agree(gi, oi, flat, off)
    assert rc == L.ERR_SYMBOL_RANGE
    stopped = 0
    for k, p in enumerate(pats):                                    # the oracle, pattern by pattern
        try:
            want = oi.search(p)
            stopped += 1
        except O.OracleError:
            want = (0, 0)
        assert (int(s[k]), int(e[k])) == want, (k, p)
    assert 0 < stopped < len(pats)                                  # both outcomes occur
    gi.close()


@pytest.mark.parametrize("variant", ["plain", "pair-kmer"])
def test_refinement_and_refusals(variant):
    t = W.dna_text_np(20000, 3)
    gi = F.FMIndex(F.Text.with_max_character(t, 4), **VARIANTS[variant])
    oi = O.OracleIndex(t, 4)
    flat, off, _ = W.substring_patterns_np(t, 500, 6, 4)
    first = gi.search_many_packed(*F.pack2(flat=flat, off=off))
    se = np.stack([first.s, first.e], axis=1).reshape(-1)
    flat2, off2 = W.ragged_patterns_np(500, 40, 4, 5)
    rc, s, e = agree(gi, oi, flat2, off2, se)                       # wrapper.rs:99-124 from (s, e)
    assert rc == L.OK
    words, _ = F.pack2(flat=flat2, off=off2)
    for what in ("backwards", "leaves", "start"):
        o, q = off2.copy(), se.copy()
        if what == "backwards":                                     # pattern 7 ends before it begins
            o[8] = o[7] - np.uint64(2)
            refused = {7}
        elif what == "leaves":                                      # entry 8 beyond off[npat]: patterns 7 and 8
            o[8] = o[-1] + np.uint64(5)
            refused = {7, 8}
        else:
            q[2 * 7] = len(t) + 1
            refused = {7}
        rp, ps, pe, pc = call(gi, "fmx_count_batch_packed2", words, o, q)
        rb, bs, be, bc = call(gi, "fmx_count_batch", flat2, o, q)
        assert rp == rb == L.ERR_ARG
        assert (ps == bs).all() and (pe == be).all() and (pc == bc).all()
        for k in range(len(o) - 1):
            if k in refused:
                assert ps[k] == pe[k] == pc[k] == 0
            elif what != "backwards" or k != 8:                     # (pattern 8 of `backwards` grew by two symbols)
                assert ps[k] == s[k] and pe[k] == e[k]
    import torch
    d = torch.zeros(64, dtype=torch.int64, device="cuda")
    args = (d.data_ptr() + 64, 1, None, d.data_ptr() + 128, None, None, None)
    assert gi._lib.fmx_count_batch_packed2_dev(gi.handle(), d.data_ptr() + 4, *args) == L.ERR_ARG
    assert gi._lib.fmx_count_batch_packed2_dev(gi.handle(), d.data_ptr(), *args) == L.OK
    torch.cuda.synchronize()
    assert gi._lib.fmx_stream_status(gi.handle()) == L.OK
    gi.close()


@pytest.mark.parametrize("make", [
    lambda t, b: F.RLFMIndex(F.Text.with_max_character(t, 4)),
    lambda t, b: F.FMIndexMultiPieces(F.Text.with_max_character(t, 4)),
    lambda t, b: F.FMIndex(F.Text.with_max_character(b, 200)),
    lambda t, b: F.FMIndex(F.Text.with_max_character(t, 4), force_wide=True),
], ids=["rlfm", "multi-pieces", "sigma-200", "wide"])
def test_other_indexes_are_refused_and_nothing_is_written(make):
    b = (W.splitmix64_np(9, 0, 3000) % np.uint64(200)).astype(np.uint8) + 1
    b[-1] = 0
    gi = make(W.dna_text_np(3000, 8), b)
    assert not gi.packed2_supported()
    flat, off = W.ragged_patterns_np(50, 9, 4, 10)
    words, _ = F.pack2(flat=flat, off=off)
    rc, s, e, c = call(gi, "fmx_count_batch_packed2", words, off)
    assert rc == L.ERR_UNSUPPORTED and (s == CANARY).all() and (e == CANARY).all() and (c == CANARY).all()
    with pytest.raises(F.Error) as ei:
        gi.search_many_packed(words, off)
    assert ei.value.code == L.ERR_UNSUPPORTED
    gi.close()


def test_pack2_round_trip_and_range():
    flat, off = W.ragged_patterns_np(200, 70, 4, 77)
    off = off + np.uint64(45)                                       # a slice: absolute numbering
    flat = np.concatenate([np.zeros(45, dtype=np.uint8), flat])     # (what lies in front of it is not looked at)
    words, off2 = F.pack2(flat=flat, off=off)
    assert words.dtype == np.uint64 and (off2 == off).all() and len(words) == (int(off[-1]) + 31) // 32
    i = np.arange(int(off[0]), int(off[-1]), dtype=np.uint64)
    unpacked = ((words[i >> np.uint64(5)] >> (np.uint64(2) * (i & np.uint64(31)))) & np.uint64(3)) + np.uint64(1)
    assert (unpacked == flat[int(off[0]):int(off[-1])]).all()
    for bad in (0, 5):
        with pytest.raises(ValueError):
            F.pack2([bytes([1, 2, bad, 4])])
