"""Both strands of 2-bit packed DNA patterns in one call (fmx_count_batch_packed2_rc / search_many_packed_both_strands):
slot 2k against the oracle and the byte call on the pattern's bytes, slot 2k + 1 against both on the bytes of its reverse
complement R (built here by plain numpy: reversed, 5 - s), for every kernel the dispatch can pick."""
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


def call(gi, name, pat, off, strands=1):
    """the C call itself: (code, s, e, count) -- the arrays come back whatever the code is"""
    nout = strands * (len(off) - 1)
    s, e, c = (np.full(max(nout, 1), CANARY, dtype=np.uint64) for _ in range(3))
    mid = () if strands == 2 else (None,)                           # the both-strand call has no s0e0
    rc = getattr(gi._lib, name)(gi.handle(), _p(pat), _p(off), len(off) - 1, *mid, _p(s), _p(e), _p(c))
    return rc, s[:nout], e[:nout], c[:nout]


def revcomp(flat, off):
    r = flat.copy()
    for a, b in zip(off[:-1].astype(np.int64), off[1:].astype(np.int64)):
        r[a:b] = 5 - flat[a:b][::-1]
    return r


def agree(gi, oi, flat, off, words=None):
    """every slot == the oracle and the byte call on that strand's bytes; even slots == the packed call.  -> (s, e)"""
    if words is None:
        words, _ = F.pack2(flat=flat, off=off)
    rc, s, e, c = call(gi, "fmx_count_batch_packed2_rc", words, off, strands=2)
    assert rc == L.OK, gi._lib.fmx_last_error()
    assert (c == e - s).all()
    for strand, f in ((0, flat), (1, revcomp(flat, off))):
        ws, we = oi.count_batch(f, off)
        rb, bs, be, bc = call(gi, "fmx_count_batch", f, off)
        assert rb == L.OK
        for got, want, byte in ((s, ws, bs), (e, we, be), (c, we - ws, bc)):
            assert (got[strand::2] == want).all() and (got[strand::2] == byte).all(), strand
    rp, ps, pe, pc = call(gi, "fmx_count_batch_packed2", words, off)
    assert rp == L.OK and (s[0::2] == ps).all() and (e[0::2] == pe).all() and (c[0::2] == pc).all()
    return s, e


@pytest.mark.parametrize("n", [4, 9, 130, 1000, 70001])
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_ragged_substring_and_revcomp_substring_patterns(variant, n):
    t = W.dna_text_np(n, 300 + n)
    gi = F.FMIndex(F.Text.with_max_character(t, 4), **VARIANTS[variant])
    oi = O.OracleIndex(t, 4)
    assert gi.packed2_rc_supported()
    assert gi.has_pair_index() == ("pair" in variant and n >= 4)
    flat, off = W.ragged_patterns_np(3000, 70, 4, 310 + n)          # empty, odd, even; refills at 32 and 64
    s, e = agree(gi, oi, flat, off)
    if n >= 130:
        for m in (31, 32, 33, 64, 65):                              # long matches through every window boundary ...
            sflat, soff, _ = W.substring_patterns_np(t, 300, m, 320 + n + m)
            for strand, f in ((0, sflat), (1, revcomp(sflat, soff))):   # ... of the strand that is certain to match
                ss, se = agree(gi, oi, f, soff)
                assert (se[strand::2] > ss[strand::2]).all()
    b = gi.search_many_packed_both_strands(*F.pack2(flat=flat, off=off))   # the Python surface: the same arrays
    assert len(b.s) == 2 * (len(off) - 1) and (b.s == s).all() and (b.e == e).all() and (b.counts == e - s).all()
    gi.close()


@pytest.mark.parametrize("variant", ["plain-kmer", "pair-kmer"])
def test_every_alignment_and_foreign_bits(variant):
    """a pattern starts and one ends at every offset mod 32, one of length 1 sits in the last 2 bits of a word; even
    patterns are text substrings, odd ones reverse complements of text substrings, every 97th symbol is changed; the
    batch as it is and as a slice from symbol 37, the bits that belong to no pattern all 0 and all 1"""
    t = W.dna_text_np(5000, 41)
    gi = F.FMIndex(F.Text.with_max_character(t, 4), **VARIANTS[variant])
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
    flat[q] = flat[q] % 4 + 1                                       # some end early
    rs, re_ = agree(gi, oi, flat, off)
    for strand in (0, 1):                                           # both outcomes on each strand
        assert (re_[strand::2] > rs[strand::2]).any() and (re_[strand::2] == rs[strand::2]).any()
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
            s, e = agree(gi, oi, f, o, words=w)
            assert (s == rs).all() and (e == re_).all()
    gi.close()


@pytest.mark.parametrize("pair", [False, True])
def test_three_bit_table_codes(pair):
    t = (W.splitmix64_np(12, 0, 5000) % np.uint64(5)).astype(np.uint8) + 1
    t[-1] = 0
    gi = F.FMIndex(F.Text.with_max_character(t, 5), pair_index=pair, kmer_table=True, plain=not pair)
    oi = O.OracleIndex(t, 5)
    assert gi.packed2_rc_supported() and gi.kmer_k() >= 2
    flat, off = W.ragged_patterns_np(2000, 40, 4, 13)               # patterns over 1..4 in a text over 1..5
    s, e = agree(gi, oi, flat, off)
    assert (e[0::2] > s[0::2]).any() and (e[1::2] > s[1::2]).any()
    gi.close()


@pytest.mark.parametrize("make", [
    lambda t, b: F.RLFMIndex(F.Text.with_max_character(t, 4)),
    lambda t, b: F.FMIndexMultiPieces(F.Text.with_max_character(t, 4)),
    lambda t, b: F.FMIndex(F.Text.with_max_character(b, 200)),
    lambda t, b: F.FMIndex(F.Text.with_max_character(t, 4), force_wide=True),
    lambda t, b: F.FMIndex(F.Text.with_max_character(np.minimum(t, 2), 2), plain=True, kmer_table=True),
    lambda t, b: F.FMIndex(F.Text.with_max_character(np.minimum(t, 3), 3), pair_index=True),
], ids=["rlfm", "multi-pieces", "sigma-200", "wide", "sigma-2", "sigma-3"])
def test_other_indexes_are_refused_and_nothing_is_written(make):
    b = (W.splitmix64_np(9, 0, 3000) % np.uint64(200)).astype(np.uint8) + 1
    b[-1] = 0
    gi = make(W.dna_text_np(3000, 8), b)
    assert not gi.packed2_rc_supported()
    flat, off = W.ragged_patterns_np(50, 9, 4, 10)
    words, _ = F.pack2(flat=flat, off=off)
    rc, s, e, c = call(gi, "fmx_count_batch_packed2_rc", words, off, strands=2)
    assert len(s) == 100 and rc == L.ERR_UNSUPPORTED
    assert (s == CANARY).all() and (e == CANARY).all() and (c == CANARY).all()
    with pytest.raises(F.Error) as ei:
        gi.search_many_packed_both_strands(words, off)
    assert ei.value.code == L.ERR_UNSUPPORTED
    gi.close()


@pytest.mark.parametrize("variant", ["plain", "pair-kmer"])
def test_bad_offsets_and_alignment(variant):
    t = W.dna_text_np(20000, 3)
    gi = F.FMIndex(F.Text.with_max_character(t, 4), **VARIANTS[variant])
    flat, off = W.ragged_patterns_np(500, 40, 4, 5)
    words, _ = F.pack2(flat=flat, off=off)
    s, e = agree(gi, O.OracleIndex(t, 4), flat, off)
    for what, refused in (("backwards", {7}), ("leaves", {7, 8})):
        o = off.copy()
        o[8] = o[7] - np.uint64(2) if what == "backwards" else o[-1] + np.uint64(5)
        rc, bs, be, bc = call(gi, "fmx_count_batch_packed2_rc", words, o, strands=2)
        assert rc == L.ERR_ARG
        for v in range(2 * (len(o) - 1)):
            if v // 2 in refused:
                assert bs[v] == be[v] == bc[v] == 0
            elif what != "backwards" or v // 2 != 8:                # (pattern 8 of `backwards` grew by two symbols)
                assert bs[v] == s[v] and be[v] == e[v] and bc[v] == e[v] - s[v]
    import torch
    d = torch.zeros(64, dtype=torch.int64, device="cuda")
    args = (d.data_ptr() + 64, 1, d.data_ptr() + 128, None, None, None)
    assert gi._lib.fmx_count_batch_packed2_rc_dev(gi.handle(), d.data_ptr() + 4, *args) == L.ERR_ARG
    assert gi._lib.fmx_count_batch_packed2_rc_dev(gi.handle(), d.data_ptr(), *args) == L.OK
    torch.cuda.synchronize()
    assert gi._lib.fmx_stream_status(gi.handle()) == L.OK
    gi.close()
