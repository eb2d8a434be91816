"""Matching statistics and SMEM seeds on 2-bit packed DNA patterns, one strand or both (fmx_match_stats_batch_packed2 /
_rc, match_stats_many_packed / _both_strands): every comparison against the loop of the header on the CPU oracle
(tests/match_stats_expect.py) AND against the byte call fmx_match_stats_batch, both on the unpacked bytes of the
virtual batch -- the patterns themselves, or P_0, R_0, P_1, R_1, ... with R built here by plain numpy."""
import ctypes as C

import numpy as np
import pytest

import fm_index_amd as F
from fm_index_amd import _lib as L
from fm_index_amd import workload as W
from oracle import fm_oracle as O
from match_stats_expect import expect_match_stats, seeds_of

pytestmark = pytest.mark.gpu

VARIANTS = {"plain": dict(plain=True), "pair": dict(pair_index=True), "plain-kmer": dict(plain=True, kmer_table=True),
            "pair-kmer": dict(pair_index=True, kmer_table=True)}
NAME = {1: "fmx_match_stats_batch_packed2", 2: "fmx_match_stats_batch_packed2_rc"}
CANARY = np.uint64(0xC0FFEE0DDBA11)
PAD = 16


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def call(gi, name, pat, off, nslot, p=(1, 0, 0), want=(True, True, True)):
    """the C call itself, every array all canaries and PAD more on either side: (code, len, s, e), whatever the code"""
    bufs = [np.full(nslot + 2 * PAD, CANARY, dtype=np.uint64) if on else None for on in want]
    v = [None if b is None else b[PAD:] for b in bufs]
    rc = getattr(gi._lib, name)(gi.handle(), _p(pat), _p(off), len(off) - 1, *[int(x) for x in p], _p(v[1]), _p(v[2]),
                                _p(v[0]))
    for b in bufs:
        assert b is None or ((b[:PAD] == CANARY).all() and (b[PAD + nslot:] == CANARY).all()), "canary overwritten"
    return (rc,) + tuple(None if b is None else b[PAD:PAD + nslot] for b in bufs)


def revcomp(p):
    return (5 - p[::-1]).astype(np.uint8)


def virtual(flat, off, strands):
    """bytes and offsets (from 0) of the batch the call answers: the patterns, or P_0, R_0, P_1, R_1, ..."""
    pats = [flat[a:b] for a, b in zip(off[:-1].astype(np.int64), off[1:].astype(np.int64))]
    if strands == 2:
        pats = [q for p in pats for q in (p, revcomp(p))]
    return F.pack_patterns(pats, np.uint8) if pats else (np.zeros(1, dtype=np.uint8), np.zeros(1, dtype=np.uint64))


def agree(gi, oi, flat, off, strands, p, words=None):
    """the packed call == the expectation == the byte call on the virtual batch; -> (len, s, e)"""
    words = F.pack2(flat=flat, off=off)[0] if words is None else words
    vf, vo = virtual(flat, off, strands)
    got = call(gi, NAME[strands], words, off, int(vo[-1]), p)
    byte = call(gi, "fmx_match_stats_batch", vf, vo, int(vo[-1]), p)
    assert got[0] == L.OK and byte[0] == L.OK, gi._lib.fmx_last_error()
    for g, w, b in zip(got[1:], expect_match_stats(oi, vf, vo, *p), byte[1:]):
        assert (g == w).all() and (g == b).all(), (strands, p, int(np.nonzero((g != w) | (g != b))[0][0]))
    return got[1:]


@pytest.mark.parametrize("strands", [1, 2])
@pytest.mark.parametrize("n", [4, 9, 130, 1000, 70001])
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_parity(variant, n, strands):
    t = W.dna_text_np(n, 500 + n)
    gi = F.FMIndex(F.Text.with_max_character(t, 4), **VARIANTS[variant])
    oi = O.OracleIndex(t, 4)
    assert gi.has_pair_index() == ("pair" in variant and n >= 4)
    if "kmer" in variant and n >= 1000:
        assert gi.kmer_k() >= 2
    k = gi.kmer_k() or 6
    flat, off = W.ragged_patterns_np(400, 70, 4, 510 + n)           # empty, odd, even; past 32 and 64
    pats = [flat[a:b] for a, b in zip(off[:-1].astype(np.int64), off[1:].astype(np.int64))]
    if n >= 130:                                                    # long matches through every window boundary ...
        for m in (31, 32, 33, 64, 65):
            sub = list(W.substring_patterns_np(t, 12, m, 520 + n + m)[0].reshape(12, m))
            pats += sub + ([revcomp(q) for q in sub] if strands == 2 else [])   # ... on each strand
    flat, off = F.pack_patterns(pats, np.uint8)
    for p in ((1, 0, 0), (2, 0, 0), (1, k - 1, 0), (1, k, 0), (1, 33, 0), (1, 0, 5), (3, 20, 8)):
        got = agree(gi, oi, flat, off, strands, p)
        ln, s, e = got if p == (1, 0, 5) else (ln, s, e) if p != (1, 0, 0) else got
        if p == (1, 0, 0) and n >= 130:
            vo = virtual(flat, off, strands)[1].astype(np.int64)
            odd = (np.searchsorted(vo, np.arange(len(ln)), side="right") - 1) % 2 == 1
            assert (ln[~odd] > 32).any() and (strands == 1 or (ln[odd] > 32).any())
    m = getattr(gi, "match_stats_many_packed" + ("_both_strands" if strands == 2 else ""))
    b = m(*F.pack2(flat=flat, off=off), min_count=1, max_len=0, min_seed_len=5)    # the Python surface: the same arrays
    vo = virtual(flat, off, strands)[1]
    assert (b.lengths == ln).all() and (b.s == s).all() and (b.e == e).all() and (b.offsets == vo).all()
    assert [tuple(int(x) for x in q) for q in b.seeds()] == seeds_of(vo, ln, s, e)
    gi.close()


@pytest.mark.parametrize("strands", [1, 2])
@pytest.mark.parametrize("variant", ["plain-kmer", "pair-kmer"])
def test_every_alignment_and_foreign_bits(variant, strands):
    """a pattern starts and one ends at every offset mod 32, one of length 1 sits in the last 2 bits of a word; the
    batch as it is and as a slice from symbol 37, the bits that belong to no pattern all 0 and all 1"""
    t = W.dna_text_np(5000, 41)
    gi = F.FMIndex(F.Text.with_max_character(t, 4), **VARIANTS[variant])
    oi = O.OracleIndex(t, 4)
    lens = [31, 1] + [33 + k % 3 for k in range(96)] + [0, 1, 2, 64]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    assert int(off[2]) == 32 and int(off[1]) == 31                  # pattern 1: one symbol in the last 2 bits of word 0
    assert {int(o) % 32 for o in off[:-1]} == set(range(32)) and {int(o) % 32 for o in off[1:]} == set(range(32))
    flat = W.substring_patterns_np(t, 1, int(off[-1]), 43)[0]
    for k in range(1, len(lens), 2):                                # odd patterns match on the other strand
        flat[int(off[k]):int(off[k + 1])] = revcomp(flat[int(off[k]):int(off[k + 1])])
    q = np.arange(50, len(flat), 97)
    flat[q] = flat[q] % 4 + 1                                       # some end early
    first = agree(gi, oi, flat, off, strands, (1, 0, 5))
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
            assert all((g == h).all() for g, h in zip(agree(gi, oi, f, o, strands, (1, 0, 5), words=w), first))
    gi.close()


@pytest.mark.parametrize("maxc,pair,strands", [(5, False, 1), (5, False, 2), (5, True, 1), (5, True, 2),
                                               (2, False, 1), (3, False, 1), (3, True, 1)])
def test_alphabets(maxc, pair, strands):
    """3-bit table codes (max_character 5); alphabets of 2 and 3 symbols, where a code that is no symbol ends the match"""
    t = (W.splitmix64_np(12, 0, 5000) % np.uint64(maxc)).astype(np.uint8) + 1
    t[-1] = 0
    gi = F.FMIndex(F.Text.with_max_character(t, maxc), pair_index=pair, kmer_table=True, plain=not pair)
    assert gi.kmer_k() >= 2 and (gi.packed2_rc_supported() if strands == 2 else gi.packed2_supported())
    flat, off = W.ragged_patterns_np(600, 40, 4, 13)                # patterns over 1..4
    for p in ((1, 0, 0), (2, 9, 3)):
        ln, s, e = agree(gi, O.OracleIndex(t, maxc), flat, off, strands, p)
        assert (ln >= gi.kmer_k()).any() and (maxc >= 4 or (ln == 0).any())
    gi.close()


REFUSED = {
    "rlfm": lambda t, b: F.RLFMIndex(F.Text.with_max_character(t, 4)),
    "multi-pieces": lambda t, b: F.FMIndexMultiPieces(F.Text.with_max_character(t, 4)),
    "sigma-200": lambda t, b: F.FMIndex(F.Text.with_max_character(b, 200)),
    "wide": lambda t, b: F.FMIndex(F.Text.with_max_character(t, 4), force_wide=True),
    "sigma-2": lambda t, b: F.FMIndex(F.Text.with_max_character(np.minimum(t, 2), 2), plain=True, kmer_table=True),
    "sigma-3": lambda t, b: F.FMIndex(F.Text.with_max_character(np.minimum(t, 3), 3), pair_index=True)}


@pytest.mark.parametrize("which,strands", [(w, st) for st in (1, 2) for w in REFUSED
                                           if st == 2 or not w.startswith("sigma-")])
def test_other_indexes_are_refused_and_nothing_is_written(which, strands):
    """(the single-strand call serves the alphabets of 2 and 3 symbols: test_alphabets)"""
    make = REFUSED[which]
    b = (W.splitmix64_np(9, 0, 3000) % np.uint64(200)).astype(np.uint8) + 1
    b[-1] = 0
    gi = make(W.dna_text_np(3000, 8), b)
    flat, off = W.ragged_patterns_np(50, 9, 4, 10)
    words, _ = F.pack2(flat=flat, off=off)
    rc, ln, s, e = call(gi, NAME[strands], words, off, strands * int(off[-1]))
    assert rc == L.ERR_UNSUPPORTED and (ln == CANARY).all() and (s == CANARY).all() and (e == CANARY).all()
    with pytest.raises(F.Error) as ei:
        getattr(gi, "match_stats_many_packed" + ("_both_strands" if strands == 2 else ""))(words, off)
    assert ei.value.code == L.ERR_UNSUPPORTED
    gi.close()


@pytest.mark.parametrize("strands", [1, 2])
@pytest.mark.parametrize("variant", ["plain", "pair-kmer"])
def test_errors(variant, strands):
    import torch
    t = W.dna_text_np(20000, 3)
    gi = F.FMIndex(F.Text.with_max_character(t, 4), **VARIANTS[variant])
    oi = O.OracleIndex(t, 4)
    flat, off = W.ragged_patterns_np(300, 40, 4, 5)
    words, _ = F.pack2(flat=flat, off=off)
    nslot = strands * int(off[-1])
    clean = agree(gi, oi, flat, off, strands, (1, 0, 3))
    r = off.astype(np.int64)
    # pattern 7 leaves the span and pattern 8 goes backwards: both refused, their slots of both strands are 0; pattern 7
    # alone goes backwards: it has no slot, and pattern 8, two symbols longer, takes slots of patterns 6 and 7
    for o8, lo, hi, zero in ((off[-1] + np.uint64(5), r[7], r[9], True), (off[7] - np.uint64(2), r[7] - 2, r[9], False)):
        o = off.copy()
        o[8] = o8
        rc, *bad = call(gi, NAME[strands], words, o, nslot, (1, 0, 3))
        assert rc == L.ERR_ARG
        for g, c in zip(bad, clean):
            assert (g[:strands * lo] == c[:strands * lo]).all() and (g[strands * hi:] == c[strands * hi:]).all()
            assert not (zero and g[strands * lo:strands * hi].any())
    # out_len == NULL is refused before anything is launched; out_s / out_e may be NULL
    rc, none, s, e = call(gi, NAME[strands], words, off, nslot, want=(False, True, True))
    assert rc == L.ERR_ARG and (s == CANARY).all() and (e == CANARY).all()
    rc, ln, none, none = call(gi, NAME[strands], words, off, nslot, (1, 0, 3), want=(True, False, False))
    assert rc == L.OK and (ln == clean[0]).all()
    # the dev form: total_syms off by one, a pointer misaligned by 4, twice on a stream into the same arrays
    d_w = torch.from_numpy(np.concatenate([words, words[:1]]).view(np.int64)).cuda()
    d_o = torch.from_numpy(off.view(np.int64)).cuda()
    out = [torch.from_numpy(np.full(nslot + 2 * PAD, CANARY, dtype=np.uint64).view(np.int64)).cuda() for _ in range(3)]
    st = torch.cuda.Stream()
    dev = getattr(gi._lib, NAME[strands] + "_dev")

    def run(wptr, total):
        torch.cuda.synchronize()
        rc = dev(gi.handle(), wptr, d_o.data_ptr(), len(off) - 1, total, 1, 0, 3, out[1].data_ptr() + 8 * PAD,
                 out[2].data_ptr() + 8 * PAD, out[0].data_ptr() + 8 * PAD, st.cuda_stream)
        torch.cuda.synchronize()
        return rc, gi._lib.fmx_stream_status(gi.handle()), [x.cpu().numpy().view(np.uint64) for x in out]

    rc, status, arr = run(d_w.data_ptr() + 4, int(off[-1]))
    assert rc == L.ERR_ARG and status == L.OK and all((a == CANARY).all() for a in arr)
    for _ in range(2):
        rc, status, arr = run(d_w.data_ptr(), int(off[-1]))
        assert rc == L.OK and status == L.OK
        for a, c in zip(arr, clean):
            assert (a[PAD:PAD + nslot] == c).all() and (a[:PAD] == CANARY).all() and (a[PAD + nslot:] == CANARY).all()
    for x in out:
        x.fill_(int(CANARY))
    rc, status, arr = run(d_w.data_ptr(), int(off[-1]) - 1)
    assert rc == L.OK and status == L.ERR_ARG and all((a[PAD + nslot - strands:] == CANARY).all() for a in arr)
    gi.close()


@pytest.mark.parametrize("strands", [1, 2])
def test_empty_text_no_patterns_and_empty_patterns(strands):
    flat, off = F.pack_patterns([np.array(p, dtype=np.uint8) for p in ([1], [], [1, 2], [4])], np.uint8)
    words, _ = F.pack2(flat=flat, off=off)
    gi = F.FMIndex(F.Text.with_max_character(np.zeros(0, dtype=np.uint8), 4))
    for msl in (0, 1):
        rc, ln, s, e = call(gi, NAME[strands], words, off, strands * 4, (1, 0, msl))
        assert rc == L.OK and not ln.any() and not s.any() and not e.any()
    o = off.copy()
    o[2] = 0
    rc, ln, s, e = call(gi, NAME[strands], words, o, strands * 4)
    assert rc == L.ERR_ARG and not ln.any() and not s.any() and not e.any()
    gi.close()
    gi = F.FMIndex(F.Text.with_max_character(W.dna_text_np(1000, 5), 4))
    for o in (np.zeros(1, dtype=np.uint64), np.full(4, 7, dtype=np.uint64)):    # npat == 0; all patterns empty
        rc, ln, s, e = call(gi, NAME[strands], words, o, 0, (1, 0, 1))
        assert rc == L.OK and len(ln) == 0
    m = getattr(gi, "match_stats_many_packed" + ("_both_strands" if strands == 2 else ""))
    b = m(words, np.zeros(1, dtype=np.uint64))
    assert len(b.lengths) == 0 and len(b.seeds()) == 0 and b.offsets.tolist() == [0]
    gi.close()


@pytest.mark.parametrize("strands", [1, 2])
@pytest.mark.parametrize("variant", ["plain", "pair-kmer"])
def test_groups_take_several_slots(variant, strands):
    """the grid is capped at 2048 blocks x 32 groups: more than 2 x 65536 slots, and no multiple of 65536"""
    n, m, cap = 1 << 16, 19, 65536
    t = W.dna_text_np(n, 61)
    npat = (2 * cap + 12345) // (m * strands) + 1
    assert (npat * m * strands) % cap != 0 and npat * m * strands > 2 * cap
    flat, off, _ = W.substring_patterns_np(t, npat, m, 62)
    hit = np.nonzero(np.arange(npat) % 3 > 0)[0]                    # two in three with one symbol changed
    q = hit * m + (W.splitmix64_np(63, 0, len(hit)) % np.uint64(m)).astype(np.int64)
    flat[q] = flat[q] % 4 + 1
    gi = F.FMIndex(F.Text.with_max_character(t, 4), **VARIANTS[variant])
    for p in ((1, 0, 0), (2, 0, 5)):
        agree(gi, O.OracleIndex(t, 4), flat, off, strands, p)
    gi.close()
