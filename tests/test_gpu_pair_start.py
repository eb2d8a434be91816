"""The pair-index count kernel's pattern start and symbol window (fmx_count_pair_kernel): the k-mer symbols and the
symbols after them are read in one batch, a pattern's unread end lives in registers as 2-bit codes (32 symbols per
refill), a window with a symbol outside 1..4 falls back to the byte-wise step, and the result stores of a pattern are
issued after the next pattern's offsets have been taken over.  (s, e) -- or the error code -- must be those of the
plain index on the same text, and the oracle's."""
import ctypes as C

import numpy as np
import pytest

import fm_index_amd as F
from fm_index_amd import workload as W
from oracle import fm_oracle as O

pytestmark = pytest.mark.gpu

ORACLE_SAMPLE = 20000


class _Pair:
    """one text: the index under test (pair index + k-mer table), the plain index and the oracle"""

    def __init__(self, text, maxc, k):
        self.text, self.maxc, self.k = text, maxc, k
        txt = F.Text.with_max_character(text, maxc)
        self.acc = F.FMIndex(txt, pair_index=True, kmer_table=True)
        self.plain = F.FMIndex(txt, plain=True)
        self.oracle = O.OracleIndex(text, maxc)
        assert self.acc.has_pair_index() and self.acc.kmer_k() == k
        assert not self.plain.has_pair_index() and self.plain.kmer_k() == 0

    def check(self, flat, off, s0e0=None):
        """same (s, e) as the plain index over all patterns and as the oracle on a sample"""
        a = self.acc.search_many(flat=flat, off=off, s0e0=s0e0)
        p = self.plain.search_many(flat=flat, off=off, s0e0=s0e0)
        assert (a.s == p.s).all() and (a.e == p.e).all() and (a.counts == p.counts).all()
        m = min(len(off) - 1, ORACLE_SAMPLE)
        first = int(off[0])
        os_, oe = self.oracle.count_batch(flat[first:], (off[:m + 1] - off[0]).astype(np.uint64),
                                          None if s0e0 is None else s0e0[:2 * m])
        assert (a.s[:m] == os_).all() and (a.e[:m] == oe).all()
        return a

    def substrings(self, lens, seed):
        """one substring of the text per entry of `lens` (every step runs), packed back to back"""
        lens = np.asarray(lens, dtype=np.int64)
        n = len(self.text)
        pos = (W.splitmix64_np(seed, 0, len(lens)) % np.uint64(n - 1 - int(lens.max(initial=0)))).astype(np.int64)
        off = np.zeros(len(lens) + 1, dtype=np.uint64)
        off[1:] = np.cumsum(lens).astype(np.uint64)
        idx = np.repeat(pos - off[:-1].astype(np.int64), lens) + np.arange(int(off[-1]), dtype=np.int64)
        flat = self.text[idx].astype(np.uint8) if len(idx) else np.zeros(1, dtype=np.uint8)
        return flat, off

    def randoms(self, lens, seed):
        """uniform random symbols 1..max_character (early exits)"""
        lens = np.asarray(lens, dtype=np.int64)
        off = np.zeros(len(lens) + 1, dtype=np.uint64)
        off[1:] = np.cumsum(lens).astype(np.uint64)
        flat = (W.splitmix64_np(seed, 0, max(int(off[-1]), 1)) % np.uint64(self.maxc)).astype(np.uint8) + 1
        return flat, off


@pytest.fixture(scope="module")
def dna():
    return _Pair(W.dna_text_np(70001, 21), 4, 6)                 # k = 6, 2-bit k-mer codes


@pytest.fixture(scope="module")
def binary():
    n = 1 << 20
    t = (W.splitmix64_np(33, 0, n) % np.uint64(2)).astype(np.uint8) + 1
    t[-1] = 0
    return _Pair(t, 2, 16)                                        # k = 16, 1-bit codes: both halves of the k-mer load


@pytest.fixture(params=["dna", "binary"])
def ix(request, dna, binary):
    return dna if request.param == "dna" else binary


def _boundary_lengths(k):
    return sorted(set(list(range(0, 4)) + list(range(k - 1, k + 4)) + list(range(k + 31, k + 35)) +
                      list(range(k + 63, k + 67)) + [80]))


def test_length_boundaries(ix):
    lens = np.repeat(_boundary_lengths(ix.k), 48)
    ix.check(*ix.substrings(lens, 5))
    ix.check(*ix.randoms(lens, 6))


def _outcome(index, flat, off):
    try:
        b = index.search_many(flat=flat, off=off)
    except F.Error as ex:
        return ("error", ex.code)
    return ("ok", int(b.s[0]), int(b.e[0]))


def test_symbols_outside_the_alphabet_position_by_position(ix):
    present, _ = ix.substrings([40], 7)
    absent = present.copy()
    # a suffix that does not occur: the search collapses before it reaches the pattern's first symbols
    for seed in range(100):
        absent[8:], _ = ix.randoms([32], 100 + seed)
        b = ix.plain.search_many(flat=absent[20:], off=np.array([0, 20], dtype=np.uint64))
        if b.counts[0] == 0:
            break
    else:
        pytest.fail("no absent suffix found")
    off1 = np.array([0, 40], dtype=np.uint64)
    saw_error = saw_hidden = False
    for base in (present, absent):
        # symbol 0 is an ordinary symbol: all 40 variants in one batch
        var = np.tile(base, (40, 1))
        var[np.arange(40), np.arange(40)] = 0
        ix.check(var.reshape(-1), np.arange(41, dtype=np.uint64) * np.uint64(40))
        # symbol 5 (and 3 on the binary text: a 2-bit code, but above max_character) is an error where it is reached,
        # and nothing where an early exit hides it
        for bad in sorted({5, ix.maxc + 1}):
            for p in range(40):
                v = base.copy()
                v[p] = bad
                got, want = _outcome(ix.acc, v, off1), _outcome(ix.plain, v, off1)
                assert got == want, (bad, p, got, want)
                saw_error |= want[0] == "error"
                saw_hidden |= want[0] == "ok"
    assert saw_error and saw_hidden


def _dev_count(index, d_flat, off):
    """fmx_count_batch_dev on a pattern buffer that is on the device as a whole: (status, s, e)"""
    import torch
    lib, h = F._lib.lib(), index.handle()
    npat = len(off) - 1
    d_off = torch.from_numpy(np.ascontiguousarray(off, dtype=np.uint64).view(np.int64)).cuda()
    s = torch.zeros(max(npat, 1), dtype=torch.int64, device="cuda")
    e = torch.zeros_like(s)
    rc = lib.fmx_count_batch_dev(h, C.c_void_p(d_flat.data_ptr()), C.c_void_p(d_off.data_ptr()), npat, None,
                                 C.c_void_p(s.data_ptr()), C.c_void_p(e.data_ptr()), None, None)
    assert rc == 0
    torch.cuda.synchronize()
    return lib.fmx_stream_status(h), s.cpu().numpy()[:npat].astype(np.uint64), e.cpu().numpy()[:npat].astype(np.uint64)


def test_offsets_and_neighbouring_symbols(ix):
    import torch
    lens = np.arange(1, 41)
    flat, off = ix.substrings(lens, 9)
    want = ix.plain.search_many(flat=flat, off=off)
    # one pattern per call in a buffer of 9s: a window that read outside [pbeg, pend) would meet a 9
    for k, m in enumerate(lens):
        start = 5 + k % 3                                         # 5, 6, 7: no multiple of 4
        buf = np.full(start + m + (0 if k % 2 else 37), 9, dtype=np.uint8)     # every other buffer ends with the pattern
        buf[start:start + m] = flat[int(off[k]):int(off[k + 1])]
        st, s, e = _dev_count(ix.acc, torch.from_numpy(buf).cuda(), np.array([start, start + m], dtype=np.uint64))
        assert st == 0 and s[0] == want.s[k] and e[0] == want.e[k], (m, start)
    # ragged patterns back to back, pat_off[0] != 0, 9s before the first pattern; the buffer ends with the last one
    rflat, roff = ix.randoms(np.arange(300) % 41, 10)
    for fl, of in ((flat, off), (rflat, roff)):
        buf = np.concatenate([np.full(7, 9, dtype=np.uint8), fl[:int(of[-1])]])
        of7 = of + np.uint64(7)
        a = ix.check(buf, of7)                                    # host entry point
        st, s, e = _dev_count(ix.acc, torch.from_numpy(buf).cuda(), of7)
        assert st == 0 and (s == a.s).all() and (e == a.e).all()


def test_refinement_without_the_table(ix):
    lens = np.repeat(np.arange(1, 71), 6)
    whole, woff = ix.substrings(lens + 3, 11)                     # pattern + the three symbols already matched
    tails = np.concatenate([whole[int(b) - 3:int(b)] for b in woff[1:]])
    first = ix.plain.search_many(flat=tails, off=np.arange(len(lens) + 1, dtype=np.uint64) * np.uint64(3))
    se = np.stack([first.s, first.e], axis=1).reshape(-1)
    heads = np.concatenate([whole[int(a):int(b) - 3] for a, b in zip(woff[:-1], woff[1:])])
    hoff = np.zeros(len(lens) + 1, dtype=np.uint64)
    hoff[1:] = np.cumsum(lens).astype(np.uint64)
    a = ix.check(heads, hoff, s0e0=se)
    full = ix.plain.search_many(flat=whole, off=woff)
    assert (a.s == full.s).all() and (a.e == full.e).all()
    rflat, roff = ix.randoms(lens, 12)
    ix.check(rflat, roff, s0e0=se)


@pytest.mark.parametrize("npat", [1, 7, 3 * 65536 + 5])
def test_more_patterns_than_groups(ix, npat):
    """the grid caps at 65 536 groups: with 3 * 65 536 + 5 patterns every group walks three or four"""
    lens = (W.splitmix64_np(13, 0, npat) % np.uint64(41)).astype(np.int64)
    sflat, off = ix.substrings(lens, 14)
    rflat, _ = ix.randoms(lens, 15)
    # substrings (every step runs) and random patterns (early exits) alternate
    take_random = np.repeat(np.arange(npat) % 2 == 1, lens)
    flat = sflat.copy()
    flat[:len(take_random)][take_random] = rflat[:len(take_random)][take_random]
    ix.check(flat, off)
