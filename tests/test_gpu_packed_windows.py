"""Every length-k window of 2-bit packed sequences, one strand or both (fmx_count_windows_packed2 / _rc): against the CPU
oracle's count AND the packed count call, both on the EXPANDED batch -- every fitting window a pattern of its own."""
import ctypes as C

import numpy as np
import pytest

import fm_index_amd as F
from fm_index_amd import _lib as L
from fm_index_amd import workload as W
from oracle import fm_oracle as O

pytestmark = pytest.mark.gpu

VARIANTS = {"plain": dict(plain=True), "pair": dict(pair_index=True), "plain-kmer": dict(plain=True, kmer_table=True),
            "pair-kmer": dict(pair_index=True, kmer_table=True)}
NAME = {1: "fmx_count_windows_packed2", 2: "fmx_count_windows_packed2_rc"}
CANARY = np.uint64(0xC0FFEE0DDBA11)
PAD = 16


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def call(gi, strands, words, off, k, nslot, want=(True, True, True)):
    """the C call itself, every array all canaries and PAD more on either side: (code, s, e, count), whatever the code"""
    bufs = [np.full(nslot + 2 * PAD, CANARY, dtype=np.uint64) if on else None for on in want]
    v = [None if b is None else b[PAD:] for b in bufs]
    rc = getattr(gi._lib, NAME[strands])(gi.handle(), _p(words), _p(off), len(off) - 1, int(k), *[_p(x) for x in v])
    for b in bufs:
        assert b is None or ((b[:PAD] == CANARY).all() and (b[PAD + nslot:] == CANARY).all()), "canary overwritten"
    return (rc,) + tuple(None if b is None else b[PAD:PAD + nslot] for b in bufs)


def expand(flat, off, k, strands):
    """every fitting window as a pattern (W_0, R_0, W_1, ... with both strands): bytes, offsets, slots; the fit mask"""
    o = off.astype(np.int64)
    fit = np.zeros(int(o[-1] - o[0]), dtype=bool)
    for a, b in zip(o[:-1] - o[0], o[1:] - o[0]):
        fit[a:max(a, b - k + 1)] = True
    start = np.nonzero(fit)[0]
    win = flat[o[0] + start[:, None] + np.arange(k)[None, :]].astype(np.uint8)
    if strands == 2:
        win = np.stack([win, 5 - win[:, ::-1]], axis=1).reshape(-1, k)
    slot = (strands * start[:, None] + np.arange(strands)[None, :]).reshape(-1)
    return win.reshape(-1), np.arange(len(win) + 1, dtype=np.uint64) * np.uint64(k), slot, np.repeat(fit, strands)


def agree(gi, oi, flat, off, k, strands, words=None, code=L.OK):
    """the window call == the packed count call (code and arrays) == the oracle (if given) on the expanded batch"""
    words = F.pack2(flat=flat, off=off)[0] if words is None else words
    vf, vo, slot, fit = expand(flat, off, k, strands)
    got = call(gi, strands, words, off, k, len(fit))
    ps, pe, pc = (np.zeros(len(slot), dtype=np.uint64) for _ in range(3))
    prc = gi._lib.fmx_count_batch_packed2(gi.handle(), _p(F.pack2(flat=vf, off=vo)[0]), _p(vo), len(slot), None, _p(ps),
                                          _p(pe), _p(pc))
    assert got[0] == prc == code, gi._lib.fmx_last_error()
    for g, p in zip(got[1:], (ps, pe, pc)):
        assert (g[slot] == p).all() and not g[~fit].any(), (k, strands)
    if oi is not None:
        os_, oe = oi.count_batch(vf, vo)
        assert (got[1][slot] == os_).all() and (got[2][slot] == oe).all() and (got[3][slot] == oe - os_).all()
    if code == L.OK:
        b = getattr(gi, "count_windows_packed" + ("_both_strands" if strands == 2 else ""))(words, off, k)
        assert (b.s == got[1]).all() and (b.e == got[2]).all() and (b.counts == got[3]).all() and (b.valid == fit).all()
    return got[1:] + (fit,)


@pytest.mark.parametrize("strands", [1, 2])
@pytest.mark.parametrize("n", [4, 130, 5000])
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_parity(variant, n, strands):
    t = W.dna_text_np(n, 700 + n)
    gi = F.FMIndex(F.Text.with_max_character(t, 4), **VARIANTS[variant])
    oi = O.OracleIndex(t, 4)
    kk = gi.kmer_k() or 6
    ks = sorted({1, 2, kk - 1, kk, kk + 1, 31, 32, 33, 65})
    flat, off = W.ragged_patterns_np(50, 70, 4, 710 + n)            # lengths 0..70
    seqs = [flat[a:b] for a, b in zip(off[:-1].astype(np.int64), off[1:].astype(np.int64))]
    lens = [m for k in ks for m in (k - 1, k, k + 1)]               # below k, equal to k, k + 1, for every k
    seqs += [W.random_patterns_np(1, m, 4, 720 + m)[0] if m else np.zeros(0, dtype=np.uint8) for m in lens]
    if n >= 130:                                                    # long matches through the 32-symbol boundary ...
        sub = W.substring_patterns_np(t, 6, 100, 730 + n)[0].reshape(6, 100)
        sub[:, 70] = sub[:, 70] % 4 + 1                             # ... and windows that end early
        seqs += list(sub)
    flat, off = F.pack_patterns(seqs, np.uint8)
    hit = miss = False
    for k in ks:
        s, e, c, fit = agree(gi, oi, flat, off, k, strands)
        hit, miss = hit or bool((e[fit] > s[fit]).any()), miss or bool((e[fit] == s[fit]).any())
    assert hit and miss                                             # among the slots that have a window
    gi.close()


@pytest.mark.parametrize("strands", [1, 2])
@pytest.mark.parametrize("variant", ["plain-kmer", "pair-kmer"])
def test_every_alignment_and_foreign_bits(variant, strands):
    """starts and ends at every offset mod 32; as it is and as a slice from symbol 37, foreign bits all 0 and all 1"""
    t = W.dna_text_np(5000, 41)
    gi = F.FMIndex(F.Text.with_max_character(t, 4), **VARIANTS[variant])
    oi = O.OracleIndex(t, 4)
    lens = [31, 1] + [33 + k % 3 for k in range(96)] + [0, 1, 2, 64]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    assert {int(o) % 32 for o in off[:-1]} == set(range(32)) and {int(o) % 32 for o in off[1:]} == set(range(32))
    flat = W.substring_patterns_np(t, 1, int(off[-1]), 43)[0]
    q = np.arange(50, len(flat), 97)
    flat[q] = flat[q] % 4 + 1                                       # some end early
    for k in (1, gi.kmer_k(), 32, 34):
        first = agree(gi, oi, flat, off, k, strands)
        o = off + np.uint64(37)
        f = np.concatenate([np.ones(37, dtype=np.uint8), flat])
        words, _ = F.pack2(flat=f, off=o)
        unused = np.ones(32 * len(words), dtype=np.uint64)
        unused[int(o[0]):int(o[-1])] = 0
        ones = ((unused * np.uint64(3)).reshape(-1, 32) << (np.arange(32, dtype=np.uint64) * np.uint64(2))).sum(
            axis=1, dtype=np.uint64)
        assert int(o[-1]) % 32 != 0 and ones[0] == np.uint64(0xFFFFFFFFFFFFFFFF)
        for w in (words, words | ones):
            assert all((g == h).all() for g, h in zip(agree(gi, oi, f, o, k, strands, words=w), first))
    gi.close()


@pytest.mark.parametrize("pair", [False, True])
def test_three_symbols(pair):
    """a window that reaches symbol 4 > max_character: FMX_ERR_SYMBOL_RANGE and zeros; the others are the oracle's"""
    t = (W.splitmix64_np(12, 0, 5000) % np.uint64(3)).astype(np.uint8) + 1
    t[-1] = 0
    gi = F.FMIndex(F.Text.with_max_character(t, 3), pair_index=pair, kmer_table=True, plain=not pair)
    oi = O.OracleIndex(t, 3)
    assert gi.kmer_k() >= 2 and gi.packed2_supported() and not gi.packed2_rc_supported()
    flat, off = W.ragged_patterns_np(60, 60, 4, 13)
    flat = np.where(W.splitmix64_np(14, 0, len(flat)) % np.uint64(5) == 0, flat, np.minimum(flat, 3)).astype(np.uint8)
    for k in (1, gi.kmer_k(), 33):
        s, e = agree(gi, None, flat, off, k, 1, code=L.ERR_SYMBOL_RANGE)[:2]
        vf, vo, slot, fit = expand(flat, off, k, 1)
        win = vf.reshape(-1, k)
        clean, first4 = (win <= 3).all(axis=1), win[:, -1] == 4     # (the last symbol is the first one reached)
        assert first4.any() and not s[slot[first4]].any() and not e[slot[first4]].any()
        os_, oe = oi.count_batch(win[clean].reshape(-1), np.arange(clean.sum() + 1, dtype=np.uint64) * np.uint64(k))
        assert (s[slot[clean]] == os_).all() and (e[slot[clean]] == oe).all()
    gi.close()


@pytest.mark.parametrize("strands", [1, 2])
@pytest.mark.parametrize("variant", ["plain", "pair-kmer"])
def test_groups_take_several_slots(variant, strands):
    """only a group's SECOND window travels through the pipeline: more than 2 x 65536 (the grid's cap) slots"""
    t = W.dna_text_np(1 << 16, 61)
    per = 48000 // strands                                          # 144000 slots either way
    flat = W.substring_patterns_np(t, 3, per, 62)[0]
    q = np.arange(7, len(flat), 23)
    flat[q] = flat[q] % 4 + 1
    gi = F.FMIndex(F.Text.with_max_character(t, 4), **VARIANTS[variant])
    oi = O.OracleIndex(t, 4)
    for k in (gi.kmer_k() or 12, 40):
        agree(gi, oi, flat, np.array([0, per + 5, 3 * per], dtype=np.uint64), k, strands)
    gi.close()


@pytest.mark.parametrize("which,strands", [("rlfm", 1), ("rlfm", 2), ("wide", 1), ("wide", 2), ("sigma-3", 2)])
def test_other_indexes_are_refused_and_nothing_is_written(which, strands):
    t = W.dna_text_np(3000, 8)
    gi = {"rlfm": lambda: F.RLFMIndex(F.Text.with_max_character(t, 4)),
          "wide": lambda: F.FMIndex(F.Text.with_max_character(t, 4), force_wide=True),
          "sigma-3": lambda: F.FMIndex(F.Text.with_max_character(np.minimum(t, 3), 3), pair_index=True)}[which]()
    flat, off = W.ragged_patterns_np(50, 9, 4, 10)
    words, _ = F.pack2(flat=flat, off=off)
    rc, s, e, c = call(gi, strands, words, off, 3, strands * int(off[-1]))
    assert rc == L.ERR_UNSUPPORTED and gi._lib.fmx_last_error() and all((x == CANARY).all() for x in (s, e, c))
    gi.close()


@pytest.mark.parametrize("strands", [1, 2])
@pytest.mark.parametrize("variant", ["plain", "pair-kmer"])
def test_errors_and_dev_form(variant, strands):
    import torch
    t = W.dna_text_np(5000, 3)
    gi = F.FMIndex(F.Text.with_max_character(t, 4), **VARIANTS[variant])
    flat, off = W.ragged_patterns_np(100, 40, 4, 5)
    words, _ = F.pack2(flat=flat, off=off)
    k, nslot = 7, strands * int(off[-1])
    clean = agree(gi, O.OracleIndex(t, 4), flat, off, k, strands)
    for kw in (dict(k=0), dict(k=k, want=(True, True, False))):     # refused before any launch; out_s / out_e may be NULL
        rc, *arr = call(gi, strands, words, off, nslot=nslot, **kw)
        assert rc == L.ERR_ARG and all(a is None or (a == CANARY).all() for a in arr)
    rc, none, none, c = call(gi, strands, words, off, k, nslot, want=(False, False, True))
    assert rc == L.OK and (c == clean[2]).all()
    # sequence 7 leaves the span and sequence 8 goes backwards: both refused, their slots hold 0, the others are unaffected
    o = off.copy()
    o[8] = off[-1] + np.uint64(5)
    lo, hi = strands * int(off[7]), strands * int(off[9])
    rc, *bad = call(gi, strands, words, o, k, nslot)
    assert rc == L.ERR_ARG and all(not g[lo:hi].any() and (g[:lo] == w[:lo]).all() and (g[hi:] == w[hi:]).all()
                                   for g, w in zip(bad, clean))
    d_w = torch.from_numpy(np.concatenate([words, words[:1]]).view(np.int64)).cuda()   # the dev form from here on
    d_o = torch.from_numpy(off.view(np.int64)).cuda()
    out = [torch.from_numpy(np.full(nslot + 2 * PAD, CANARY, dtype=np.uint64).view(np.int64)).cuda() for _ in range(3)]
    dev = getattr(gi._lib, NAME[strands] + "_dev")

    def run(wptr, total, stream):
        return dev(gi.handle(), wptr, d_o.data_ptr(), len(off) - 1, total, k, *[x.data_ptr() + 8 * PAD for x in out], stream)

    def results():
        torch.cuda.synchronize()
        return gi._lib.fmx_stream_status(gi.handle()), [x.cpu().numpy().view(np.uint64) for x in out]

    side = torch.cuda.Stream()
    assert run(d_w.data_ptr() + 4, int(off[-1]), side.cuda_stream) == L.ERR_ARG
    status, arr = results()
    assert status == L.OK and all((a == CANARY).all() for a in arr)
    with torch.cuda.stream(side):
        assert run(d_w.data_ptr(), int(off[-1]), side.cuda_stream) == L.OK      # warm-up outside the capture
        side.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            assert run(d_w.data_ptr(), int(off[-1]), torch.cuda.current_stream().cuda_stream) == L.OK
        for _ in range(3):
            for x in out:
                x[PAD:PAD + nslot] = 12345
            g.replay()
            status, arr = results()
            assert status == L.OK and all((a[PAD:PAD + nslot] == w).all() and (a[:PAD] == CANARY).all() and
                                          (a[PAD + nslot:] == CANARY).all() for a, w in zip(arr, clean))
    out[0].fill_(int(CANARY)), out[1].fill_(int(CANARY)), out[2].fill_(int(CANARY))
    assert run(d_w.data_ptr(), int(off[-1]) - 1, side.cuda_stream) == L.OK
    status, arr = results()
    assert status == L.ERR_ARG and all((a[PAD + nslot - strands:] == CANARY).all() for a in arr)
    gi.close()


@pytest.mark.parametrize("strands", [1, 2])
def test_empty_text_and_no_sequences(strands):
    flat, off = F.pack_patterns([np.array(p, dtype=np.uint8) for p in ([1], [], [1, 2, 3], [4, 1])], np.uint8)
    words, _ = F.pack2(flat=flat, off=off)
    gi = F.FMIndex(F.Text.with_max_character(np.zeros(0, dtype=np.uint8), 4))
    rc, s, e, c = call(gi, strands, words, off, 2, strands * 6)
    assert rc == L.OK and not s.any() and not e.any() and not c.any()
    gi.close()
    gi = F.FMIndex(F.Text.with_max_character(W.dna_text_np(1000, 5), 4))
    for o in (np.zeros(1, dtype=np.uint64), np.full(4, 7, dtype=np.uint64)):    # nseq == 0; all sequences empty
        assert call(gi, strands, words, o, 2, 0)[0] == L.OK
    b = getattr(gi, "count_windows_packed" + ("_both_strands" if strands == 2 else ""))(words, off[:1], 2)
    assert len(b.counts) == 0 and len(b.valid) == 0
    gi.close()
