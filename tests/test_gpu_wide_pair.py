"""FMX_FLAG_PAIR_INDEX on the 64-bit engine (texts of 2^32 - 16 symbols or more; here force_wide=True, where a
superblock is 2^12 rows = 32 pair records = 16 one-step records, so the sizes below cross many of them).  One probe of
the 2-gram records per interval end advances two pattern symbols; (s, e, counts) must stay bit-identical to the oracle,
to the same wide index built without the flag and to the 32-bit index with the flag -- including the pair the
reference's early exit leaves (wrapper.rs:111-113) when a pair step collapses the interval."""
import ctypes as C
import struct

import numpy as np
import pytest

import fm_index_amd as F
from fm_index_amd import workload as W
from oracle import fm_oracle as O

pytestmark = pytest.mark.gpu


def _same(batch, os_, oe):
    assert (batch.s == os_).all() and (batch.e == oe).all()
    assert (batch.counts == oe - os_).all()


class _Trio:
    """oracle + wide index with the pair index + wide index without it + the 32-bit index with it, of one text"""

    def __init__(self, text, maxc, kmer_table=False):
        txt = F.Text.with_max_character(text, maxc)
        self.text = text
        self.oracle = O.OracleIndex(text, maxc)
        self.pair = F.FMIndex(txt, pair_index=True, kmer_table=kmer_table, force_wide=True)
        self.plain = F.FMIndex(txt, force_wide=True)
        self.narrow = F.FMIndex(txt, pair_index=True, kmer_table=kmer_table)
        assert self.pair.is_wide() and self.plain.is_wide() and not self.narrow.is_wide()
        assert self.pair.has_pair_index()            # (fails without the feature: the wide engine ignored the flag)
        assert not self.plain.has_pair_index() and self.narrow.has_pair_index()

    def check(self, flat, off, s0e0=None):
        os_, oe = self.oracle.count_batch(flat, off, s0e0)
        for g in (self.pair, self.plain, self.narrow):
            _same(g.search_many(flat=flat, off=off, s0e0=s0e0), os_, oe)

    def close(self):
        for g in (self.pair, self.plain, self.narrow):
            g.close()
        self.oracle.close()


@pytest.fixture(scope="module")
def dna70001():
    text = W.dna_text_np(70001, 40 + 70001)
    yield text


# the minimum n, one pair-record boundary (130), row n on either side of a superblock boundary (4095 / 4096 / 4097),
# 18 superblocks (bases in LDS: FMXW_LDS_SB = 64) and 65 (bases from global memory)
@pytest.mark.parametrize("n", [4, 5, 9, 130, 4095, 4096, 4097, 70001, (1 << 18) + 9])
def test_wide_pair_index_sizes(n, dna70001):
    trio = _Trio(dna70001 if n == 70001 else W.dna_text_np(n, 40 + n), 4)
    flat, off = W.ragged_patterns_np(3000, 13, 4, 50 + n)      # lengths 0..13: odd and even, mostly absent
    trio.check(flat, off)
    if n > 40:
        flat2, off2, _ = W.substring_patterns_np(trio.text, 2000, 17, 60 + n)
        trio.check(flat2, off2)
        flat3, off3, _ = W.substring_patterns_np(trio.text, 2000, 2, 61 + n)   # one pair step, wide ranges
        trio.check(flat3, off3)
    trio.close()


def test_wide_pair_index_every_short_pattern_including_zero_symbol():
    """all patterns of length 1..3 over {0..4}: code-0 rows, symbol 0 inside a pattern."""
    trio = _Trio(W.dna_text_np(3001, 7), 4)
    pats = []
    for m in (1, 2, 3):
        for v in range(5 ** m):
            pats.append(bytes((v // 5 ** q) % 5 for q in range(m)))
    flat, off = F.pack_patterns(pats)
    trio.check(flat, off)
    trio.close()


def test_wide_pair_index_all_equal_text_and_small_alphabet():
    # every 2-gram is code 0: its counter climbs through a whole superblock, the row0 / row1 correction in 64 bits
    t = np.array([1] * 8191 + [0], dtype=np.uint8)
    trio = _Trio(t, 4)
    flat, off = F.pack_patterns([bytes([1] * m) for m in range(0, 40)] + [bytes([1, 2]), bytes([2, 1])])
    trio.check(flat, off)
    trio.close()
    t2 = (W.splitmix64_np(5, 0, 5000) % np.uint64(2)).astype(np.uint8) + 1
    t2[-1] = 0
    trio2 = _Trio(t2, 2)                                       # max_character 2
    flat2, off2 = W.ragged_patterns_np(2000, 12, 2, 9)
    trio2.check(flat2, off2)
    flat3, off3, _ = W.substring_patterns_np(t2, 1000, 11, 10)
    trio2.check(flat3, off3)
    # a symbol of 1..4 above max_character never takes a pair step: refused where the reference reaches it
    with pytest.raises(F.Error) as ei:
        trio2.pair.search_many(flat=np.array([1, 2, 3, 1, 2], dtype=np.uint8), off=np.array([0, 5], dtype=np.uint64))
    assert ei.value.code == F._lib.ERR_SYMBOL_RANGE
    trio2.close()


def test_wide_pair_index_refinement_and_errors():
    n = 20000
    trio = _Trio(W.dna_text_np(n, 3), 4)
    flat, off, _ = W.substring_patterns_np(trio.text, 500, 5, 4)
    first = trio.plain.search_many(flat=flat, off=off)
    se = np.stack([first.s, first.e], axis=1).reshape(-1)
    flat2, off2 = W.ragged_patterns_np(500, 7, 4, 5)
    trio.check(flat2, off2, s0e0=se)                           # wrapper.rs:99-124 from (s, e)
    for p in (bytes([1, 2, 7, 1]), bytes([1, 2, 7]), bytes([7, 1, 2, 3, 4])):
        with pytest.raises(F.Error) as ei:
            trio.pair.search(p)
        assert ei.value.code == F._lib.ERR_SYMBOL_RANGE
    se_bad = np.array([0, n + 5], dtype=np.uint64)
    with pytest.raises(F.Error) as ei:
        trio.pair.search_many(flat=flat[:5], off=off[:2], s0e0=se_bad)
    assert ei.value.code == F._lib.ERR_ARG
    trio.check(flat, off)                                      # the status word was cleared
    trio.close()


def test_wide_pair_index_with_the_kmer_table(dna70001):
    trio = _Trio(dna70001, 4, kmer_table=True)
    k = trio.pair.kmer_k()
    assert k == 5 and trio.plain.kmer_k() == 0                 # 4^5 <= 70001 / 32 = 2187
    for m in (k - 1, k, k + 1, k + 2, 2 * k + 3):              # an odd and an even remainder after the table
        flat, off, _ = W.substring_patterns_np(trio.text, 3000, m, 60 + m)
        trio.check(flat, off)
    flat2, off2 = W.ragged_patterns_np(4000, 24, 4, 5)         # mostly absent k-mers: the table's early-exit pairs
    trio.check(flat2, off2)
    trio.close()


def _not_applicable(kind, text, maxc, flat, off):
    """the flag through the C ABI (the package's RLFM / multi-pieces classes do not offer it): ignored, results unchanged"""
    L = F._lib
    lib = L.lib()
    h = C.c_void_p()
    code = {"fm": L.KIND_FM, "rlfm": L.KIND_RLFM, "multi": L.KIND_MULTI}[kind]
    assert lib.fmx_build(F._p(text), len(text), text.dtype.itemsize, maxc, code, L.NO_LOCATE,
                         L.FLAG_PAIR_INDEX | L.FLAG_FORCE_WIDE, 0, C.byref(h)) == 0
    assert lib.fmx_is_wide(h) == 1 and lib.fmx_has_pair_index(h) == 0
    npat = len(off) - 1
    s, e, c = (np.zeros(npat, dtype=np.uint64) for _ in range(3))
    flat = np.ascontiguousarray(flat.astype(text.dtype))
    assert lib.fmx_count_batch(h, F._p(flat), F._p(off), npat, None, F._p(s), F._p(e), F._p(c)) == 0
    lib.fmx_free(h)
    oi = O.OracleIndex(text.astype(np.uint8), maxc, kind=kind)
    os_, oe = oi.count_batch(flat.astype(np.uint8), off)
    assert (s == os_).all() and (e == oe).all() and (c == oe - os_).all()
    oi.close()


def test_wide_pair_index_not_applicable_keeps_the_plain_kernels():
    n = 6000
    t7 = ((W.splitmix64_np(7, 0, n) % np.uint64(7)) + np.uint64(1)).astype(np.uint8)
    t7[-1] = 0
    flat7, off7 = W.ragged_patterns_np(1000, 6, 7, 3)
    _not_applicable("fm", t7, 7, flat7, off7)                  # the wide one-level kernels, but sigma > 4
    tb = W.byte_text_np(n, 4)
    flatb, offb, _ = W.substring_patterns_np(tb, 1000, 3, 5)
    _not_applicable("fm", tb, 255, flatb, offb)                # a byte alphabet
    dna = W.dna_text_np(n, 9)
    flat, off, _ = W.substring_patterns_np(dna, 1000, 7, 6)
    flatr, offr = W.ragged_patterns_np(1000, 9, 4, 8)
    tz = dna.copy()
    tz[[1500, 4001]] = 0                                       # an interior zero
    for fl, of in ((flat, off), (flatr, offr)):
        _not_applicable("fm", tz, 4, fl, of)
        _not_applicable("rlfm", dna, 4, fl, of)
        _not_applicable("multi", tz, 4, fl, of)
        _not_applicable("fm", dna.astype(np.uint16), 4, fl, of)   # u16 symbols


def test_wide_pair_index_space(dna70001):
    n = 70001
    txt = F.Text.with_max_character(dna70001, 4)
    gp = F.FMIndex(txt, pair_index=True, force_wide=True)
    g0 = F.FMIndex(txt, force_wide=True)
    extra = gp.heap_size() - g0.heap_size()
    # n bytes of records rounded up to 128, plus 128 bytes per 2^12-row superblock
    assert n <= extra <= n + n // 32 + 4096, extra
    assert extra == (n // 128 + 1) * 128 + ((n >> 12) + 1) * 128
    gp.close()
    g0.close()


def test_wide_pair_index_survives_save_load_and_damaged_files_are_refused(tmp_path):
    n = 20001
    t = W.dna_text_np(n, 8)
    g = F.FMIndexWithLocate(F.Text.with_max_character(t, 4), 2, pair_index=True, kmer_table=True, force_wide=True)
    assert g.is_wide() and g.has_pair_index() and g.kmer_k() == 4
    path = str(tmp_path / "p.fmx")
    g.save(path)
    g2 = F.FMIndexWithLocate.load(path)
    assert g2.is_wide() and g2.has_pair_index() and g2.kmer_k() == g.kmer_k() and g2.heap_size() == g.heap_size()
    oi = O.OracleIndex(t, 4, level=2)
    flat, off = W.ragged_patterns_np(3000, 20, 4, 2)
    flat2, off2, _ = W.substring_patterns_np(t, 2000, 9, 4)
    for fl, of in ((flat, off), (flat2, off2)):
        os_, oe = oi.count_batch(fl, of)
        _same(g.search_many(flat=fl, off=of), os_, oe)
        b2 = g2.search_many(flat=fl, off=of)
        _same(b2, os_, oe)
    goff, gpos = b2.locate()                                   # locate() through the loaded index is unchanged
    ooff, opos = oi.locate_batch(os_, oe)
    assert (goff == ooff).all() and (gpos == opos).all()
    g2.close()
    oi.close()
    # damaged files: load and free only -- a handle loaded from a damaged file is never queried
    raw = bytearray(open(path, "rb").read())
    lib = g._lib

    def load(buf):
        p = str(tmp_path / "y.fmx")
        open(p, "wb").write(bytes(buf))
        h = C.c_void_p()
        rc = lib.fmx_load(p.encode(), 0, C.byref(h))
        if rc == 0:
            lib.fmx_free(h)
        return rc
    assert load(raw) == 0
    # the pair index is the file's last section: pair records ((n / 128 + 1) x 128 bytes) | pair bases (128 bytes per
    # superblock)
    bases = ((n >> 12) + 1) * 128
    assert load(raw[:len(raw) - bases - 1000]) != 0            # truncated inside the pair records
    assert load(raw[:len(raw) - bases]) != 0                   # ... at their end: the bases are missing
    assert load(raw[:len(raw) - 8]) != 0                       # ... inside the bases
    assert load(raw + bytes(16)) != 0                          # trailing bytes
    # the section's own fields (32 bytes behind the device struct): presence flags that are not 1, rows above n (200 in
    # the low word of a row is a row of this index: nothing can tell it from the right one, so that file loads)
    hdr = 8 + 4 + 4 + 5 * 8 + 4 * 4
    dev_bytes = struct.unpack_from("<I", raw, 12)[0] & 0x7FFFFFFF      # (the top bit marks a wide file)
    for o in range(hdr + dev_bytes, hdr + dev_bytes + 32, 4):
        for val in (0xFFFFFFFF, 200, 0x7FFFFFF0):
            bad = bytearray(raw)
            struct.pack_into("<I", bad, o, val)
            rel = o - hdr - dev_bytes
            assert (load(bad) != 0) == (not (rel in (16, 24) and val <= n)), (rel, val)
    # an index without the flag writes the file it always wrote: no section, and claiming one is refused
    p0 = F.FMIndexWithLocate(F.Text.with_max_character(t, 4), 2, kmer_table=True, force_wide=True)
    p0.save(path)
    p0.close()
    raw0 = bytearray(open(path, "rb").read())
    assert len(raw0) == len(raw) - 32 - (n // 128 + 1) * 128 - bases
    assert load(raw0) == 0
    struct.pack_into("<I", raw0, 8, struct.unpack_from("<I", raw, 8)[0])   # the version of a file with the section
    assert load(raw0) != 0
    g.close()


def test_wide_pair_index_replicas(dna70001):
    g = F.FMIndex(F.Text.with_max_character(dna70001, 4), pair_index=True, force_wide=True)
    assert g.is_wide() and g.has_pair_index()
    reps = F.Replicas.of(g, [0, 0])
    assert all(ix.has_pair_index() and ix.is_wide() for ix in reps.indexes)
    assert all(ix.heap_size() == g.heap_size() for ix in reps.indexes)
    flat, off = W.ragged_patterns_np(3001, 20, 4, 41)
    flat2, off2, _ = W.substring_patterns_np(dna70001, 3001, 11, 43)
    oi = O.OracleIndex(dna70001, 4)
    for fl, of in ((flat, off), (flat2, off2)):
        one = g.search_many(flat=fl, off=of)
        b = reps.search_many(flat=fl, off=of)
        assert (b.s == one.s).all() and (b.e == one.e).all() and (b.counts == one.counts).all()
        os_, oe = oi.count_batch(fl, of)
        _same(b, os_, oe)
    oi.close()
    reps.close()
