"""Longest-suffix match on 2-bit packed DNA patterns, one strand or both (fmx_suffix_match_batch_packed2[_rc],
suffix_match_many_packed[_both_strands]): every slot against the loop of include/fmx.h on the CPU oracle
(tests/suffix_match_expect.py) and against the byte call on the same bytes -- odd slots on the bytes of the reverse
complement, built here by plain numpy (reversed, 5 - s) -- for every kernel the dispatch can pick."""
import ctypes as C

import numpy as np
import pytest

import fm_index_amd as F
from fm_index_amd import _lib as L
from fm_index_amd import workload as W
from oracle import fm_oracle as O
from suffix_match_expect import expect_suffix_match

pytestmark = pytest.mark.gpu

VARIANTS = {"plain": dict(plain=True), "pair": dict(pair_index=True), "pair-kmer": dict(pair_index=True, kmer_table=True),
            "plain-kmer": dict(plain=True, kmer_table=True)}
CANARY = 0xC0FFEE
ONE, BOTH = "fmx_suffix_match_batch_packed2", "fmx_suffix_match_batch_packed2_rc"


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def call(gi, name, pat, off, min_count=1, s0e0=None):
    """the C call itself: (code, u64[4, nout] = s, e, count, L) -- the arrays come back whatever the code is"""
    nout = (2 if name == BOTH else 1) * (len(off) - 1)
    out = [np.full(max(nout, 1), CANARY, dtype=np.uint64) for _ in range(4)]
    mid = () if name == BOTH else (_p(s0e0),)                       # the both-strand call has no s0e0
    rc = getattr(gi._lib, name)(gi.handle(), _p(pat), _p(off), len(off) - 1, *mid, min_count, *map(_p, out))
    return rc, np.stack(out)[:, :nout]


def revcomp(flat, off):
    r = flat.copy()
    for a, b in zip(off[:-1].astype(np.int64), off[1:].astype(np.int64)):
        r[a:b] = 5 - flat[a:b][::-1]
    return r


def agree(gi, oi, flat, off, min_count=1, words=None, both=True, s0e0=None):
    """the packed call == the oracle's loop == the byte call, on every strand asked for -> u64[4, nout]"""
    if words is None:
        words, _ = F.pack2(flat=flat, off=off)
    rc, one = call(gi, ONE, words, off, min_count, s0e0)
    assert rc == L.OK, gi._lib.fmx_last_error()
    got = one
    if both:
        rc, got = call(gi, BOTH, words, off, min_count)
        assert rc == L.OK and (got[:, 0::2] == one).all()
    for strand, f in ((0, flat), (1, revcomp(flat, off)))[:2 if both else 1]:
        want = np.stack(expect_suffix_match(oi, f, off, s0e0, min_count))
        rb, byte = call(gi, "fmx_suffix_match_batch", f, off, min_count, s0e0)
        assert rb == L.OK
        mine = got[:, strand::2] if both else got
        assert (mine == want).all() and (mine == byte).all(), (strand, min_count)
    return got


@pytest.mark.parametrize("n", [4, 9, 130, 1000, 70001])
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_ragged_substring_and_revcomp_substring_patterns(variant, n):
    t = W.dna_text_np(n, 300 + n)
    gi = F.FMIndex(F.Text.with_max_character(t, 4), **VARIANTS[variant])
    oi = O.OracleIndex(t, 4)
    assert gi.packed2_rc_supported() and gi.has_pair_index() == ("pair" in variant and n >= 4)
    flat, off = W.ragged_patterns_np(3000, 70, 4, 310 + n)          # empty, odd, even; refills at 32 and 64
    for mc in (1, 2, 50):                                           # 50: wider than the table entries of n = 70001
        r = agree(gi, oi, flat, off, mc)
        if n == 70001:
            assert (r[3] == 0).any() and (r[3] > 0).any()
    if n >= 130:                                                    # long matches through every window boundary ...
        subs = [W.substring_patterns_np(t, 60, m, 320 + n + m)[0] for m in (31, 32, 33, 64, 65)]
        soff = np.concatenate([[0], np.cumsum(np.repeat([31, 32, 33, 64, 65], 60))]).astype(np.uint64)
        sflat = np.concatenate(subs)
        for strand, f in ((0, sflat), (1, revcomp(sflat, soff))):   # ... of the strand that is certain to match
            assert (agree(gi, oi, f, soff)[3, strand::2] == soff[1:] - soff[:-1]).all()
    words, _ = F.pack2(flat=flat, off=off)                          # the Python surface: the same arrays
    for b, w in ((gi.suffix_match_many_packed_both_strands(words, off, min_count=50), r),
                 (gi.suffix_match_many_packed(words, off, min_count=50), r[:, 0::2])):
        assert (b.s == w[0]).all() and (b.e == w[1]).all() and (b.counts == w[2]).all() and (b.lengths == w[3]).all()
    gi.close()


@pytest.mark.parametrize("variant", ["plain-kmer", "pair-kmer"])
def test_every_alignment_and_foreign_bits(variant):
    """a pattern starts and one ends at every offset mod 32, one of length 1 sits in the last 2 bits of a word; even
    patterns are text substrings, odd ones reverse complements of text substrings, every 97th symbol is changed; the
    batch as it is and as a slice from symbol 37, the bits that belong to no pattern all 0 and all 1"""
    t = W.dna_text_np(5000, 41)
    gi = F.FMIndex(F.Text.with_max_character(t, 4), **VARIANTS[variant])
    oi = O.OracleIndex(t, 4)
    lens = np.array([31, 1] + [33 + k % 3 for k in range(96)] + [0, 1, 2, 64])
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    assert int(off[2]) == 32 and int(off[1]) == 31                  # pattern 1: one symbol in the last 2 bits of word 0
    assert {int(o) % 32 for o in off[:-1]} == set(range(32)) and {int(o) % 32 for o in off[1:]} == set(range(32))
    flat = W.substring_patterns_np(t, 1, int(off[-1]), 43)[0]
    other = revcomp(W.substring_patterns_np(t, 1, int(off[-1]), 44)[0], off)
    for k in range(1, len(lens), 2):
        flat[int(off[k]):int(off[k + 1])] = other[int(off[k]):int(off[k + 1])]
    q = np.arange(50, len(flat), 97)
    flat[q] = flat[q] % 4 + 1                                       # some end early
    base = agree(gi, oi, flat, off)
    for strand in (0, 1):                                           # whole and partial matches on each strand
        full = base[3, strand::2] == lens
        assert (full & (lens > 32)).any() and (~full).any()
    for lead in (0, 37):
        o = off + np.uint64(lead)
        f = np.concatenate([np.ones(lead, dtype=np.uint8), flat])
        words, _ = F.pack2(flat=f, off=o)
        unused = np.ones(32 * len(words), dtype=np.uint64)
        unused[int(o[0]):int(o[-1])] = 0
        ones = ((unused * np.uint64(3)).reshape(-1, 32) << (np.arange(32, dtype=np.uint64) * np.uint64(2))).sum(
            axis=1, dtype=np.uint64)
        assert int(o[-1]) % 32 != 0 and (lead == 0 or ones[0] == np.uint64(0xFFFFFFFFFFFFFFFF))
        for w in (words, words | ones):
            assert (agree(gi, oi, f, o, words=w) == base).all()
    gi.close()


@pytest.mark.parametrize("variant", ["plain", "pair"])
def test_start_pairs(variant):
    t = W.dna_text_np(20000, 3)
    gi = F.FMIndex(F.Text.with_max_character(t, 4), **VARIANTS[variant])
    oi = O.OracleIndex(t, 4)
    flat, off = W.ragged_patterns_np(500, 40, 4, 5)
    first = agree(gi, oi, *W.ragged_patterns_np(500, 6, 4, 6), min_count=4, both=False)
    se = np.ascontiguousarray(first[:2].T).reshape(-1)              # start pairs taken from a first search
    se[2 * 3:2 * 3 + 2] = (10, 5)                                   # e < s
    se[2 * 5:2 * 5 + 2] = (7, 8)                                    # below min_count
    good = agree(gi, oi, flat, off, min_count=2, both=False, s0e0=se)
    assert good[3, 3] == good[3, 5] == 0 and (good[3] > 0).any() and tuple(good[:3, 3]) == (10, 5, 0)
    se[2 * 9 + 1] = len(oi) + 1                                     # not a range of this index
    rc, r = call(gi, ONE, F.pack2(flat=flat, off=off)[0], off, 2, se)
    keep = np.arange(len(off) - 1) != 9
    assert rc == L.ERR_ARG and not r[:, 9].any() and (r[:, keep] == good[:, keep]).all()
    gi.close()


@pytest.mark.parametrize("sigma,pair", [(2, False), (3, True), (5, False), (5, True)])
def test_small_alphabets_and_three_bit_table_codes(sigma, pair):
    t = (W.splitmix64_np(12, 0, 5000) % np.uint64(sigma)).astype(np.uint8) + 1
    t[-1] = 0
    gi = F.FMIndex(F.Text.with_max_character(t, sigma), pair_index=pair, kmer_table=True, plain=not pair)
    oi = O.OracleIndex(t, sigma)
    assert gi.packed2_supported() and gi.packed2_rc_supported() == (sigma >= 4) and gi.kmer_k() >= 2
    flat, off = W.ragged_patterns_np(2000, 40, 4, 13)               # patterns over 1..4: codes above a small alphabet
    for mc in (1, 3):                                               # ... end the match, status OK
        r = agree(gi, oi, flat, off, mc, both=sigma >= 4)
        assert (r[3] > 0).any() and (r[3] < np.repeat(off[1:] - off[:-1], 2 if sigma >= 4 else 1)).any()
    if sigma < 4:
        rc, r = call(gi, BOTH, F.pack2(flat=flat, off=off)[0], off)
        assert rc == L.ERR_UNSUPPORTED and (r == CANARY).all()
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
    flat, off = W.ragged_patterns_np(50, 9, 4, 10)
    words, _ = F.pack2(flat=flat, off=off)
    for name, method in ((ONE, gi.suffix_match_many_packed), (BOTH, gi.suffix_match_many_packed_both_strands)):
        rc, r = call(gi, name, words, off)
        assert rc == L.ERR_UNSUPPORTED and r.shape[1] >= 50 and (r == CANARY).all()
        with pytest.raises(F.Error) as ei:
            method(words, off)
        assert ei.value.code == L.ERR_UNSUPPORTED
    gi.close()


@pytest.mark.parametrize("variant", ["plain", "pair-kmer"])
def test_bad_offsets_and_alignment(variant):
    t = W.dna_text_np(20000, 3)
    gi = F.FMIndex(F.Text.with_max_character(t, 4), **VARIANTS[variant])
    flat, off = W.ragged_patterns_np(500, 40, 4, 5)
    words, _ = F.pack2(flat=flat, off=off)
    good = agree(gi, O.OracleIndex(t, 4), flat, off)
    for what, refused in (("backwards", {7}), ("leaves", {7, 8})):
        o = off.copy()
        o[8] = o[7] - np.uint64(2) if what == "backwards" else o[-1] + np.uint64(5)
        for name, want in ((ONE, good[:, 0::2]), (BOTH, good)):
            rc, r = call(gi, name, words, o)
            per = r.shape[1] // (len(o) - 1)
            pat = np.arange(r.shape[1]) // per
            keep = ~np.isin(pat, list(refused | {8}))               # (pattern 8 of `backwards` grew by two symbols)
            assert rc == L.ERR_ARG and not r[:, np.isin(pat, list(refused))].any()
            assert (r[:, keep] == want[:, keep]).all()
    import torch
    d = torch.zeros(64, dtype=torch.int64, device="cuda")
    for name, mid in ((ONE, (None, 1)), (BOTH, (1,))):
        fn = getattr(gi._lib, name + "_dev")
        args = (d.data_ptr() + 64, 1, *mid, d.data_ptr() + 128, None, None, d.data_ptr() + 256, None)
        assert fn(gi.handle(), d.data_ptr() + 4, *args) == L.ERR_ARG
        assert fn(gi.handle(), d.data_ptr(), *args) == L.OK
        torch.cuda.synchronize()
        assert gi._lib.fmx_stream_status(gi.handle()) == L.OK
    gi.close()


@pytest.mark.parametrize("name", [ONE, BOTH])
def test_empty_text_and_no_patterns(name):
    flat, off = F.pack_patterns([np.array(p, dtype=np.uint8) for p in ([1], [], [1, 2], [4])], np.uint8)
    words, _ = F.pack2(flat=flat, off=off)
    gi = F.FMIndex(F.Text.with_max_character(np.zeros(0, dtype=np.uint8), 4))
    rc, r = call(gi, name, words, off)
    assert rc == L.OK and r.shape[1] in (4, 8) and not r.any()
    o = off.copy()
    o[2] = 0                                                        # the offsets are still checked
    rc, r = call(gi, name, words, o)
    assert rc == L.ERR_ARG and not r.any()
    gi.close()
    gi = F.FMIndex(F.Text.with_max_character(W.dna_text_np(1000, 5), 4))
    rc, r = call(gi, name, None, np.zeros(1, dtype=np.uint64))      # npat == 0: nothing is written
    assert rc == L.OK and r.shape == (4, 0)
    gi.close()
