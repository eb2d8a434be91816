"""FMX_FLAG_KMER_TABLE on the 64-bit engine (texts of 2^32 - 16 symbols or more; here force_wide=True, where a
superblock is 2^12 rows, so every shape crosses many of them).  A fresh pattern's first k steps come from one 16-byte
table entry; (s, e, counts) must stay bit-identical to the oracle, to the same wide index built without the flag and
to the 32-bit index with the flag -- including the equal pair the reference's early exit leaves (wrapper.rs:111-113)
when the k-mer itself does not occur.  k = min(floor(24 / bits), 16) reduced while 2^(bits k) > n / 32."""
import ctypes as C
import struct

import numpy as np
import pytest

import fm_index_amd as F
from fm_index_amd import workload as W
from oracle import fm_oracle as O

pytestmark = pytest.mark.gpu

_CLS = {"fm": F.FMIndex, "rlfm": F.RLFMIndex, "multi": F.FMIndexMultiPieces}


def _same(batch, os_, oe):
    assert (batch.s == os_).all() and (batch.e == oe).all()
    assert (batch.counts == oe - os_).all()


class _Trio:
    """oracle + wide index with the table + wide index without it (+ the 32-bit index with the table) of one text"""

    def __init__(self, text, maxc, kind="fm", narrow=True):
        txt = F.Text.with_max_character(text, maxc)
        cls = _CLS[kind]
        self.text = text
        self.oracle = O.OracleIndex(text, maxc, kind=kind)
        self.table = cls(txt, kmer_table=True, force_wide=True)
        self.plain = cls(txt, force_wide=True)
        self.narrow = cls(txt, kmer_table=True) if narrow else None
        assert self.table.is_wide() and self.plain.is_wide()
        assert self.plain.kmer_k() == 0

    def check(self, flat, off, s0e0=None):
        os_, oe = self.oracle.count_batch(flat, off, s0e0)
        for g in (self.table, self.plain, self.narrow):
            if g is not None:
                _same(g.search_many(flat=flat, off=off, s0e0=s0e0), os_, oe)

    def close(self):
        for g in (self.table, self.plain, self.narrow):
            if g is not None:
                g.close()
        self.oracle.close()


@pytest.fixture(scope="module")
def dna70001():
    t = _Trio(W.dna_text_np(70001, 11 + 70001), 4)
    yield t
    t.close()


# n / 32 = 2187, 8192, 34, 9 entries at the most -> 4^5, 4^6, 4^2, none; 18 superblocks keep their bases in LDS
# (FMXW_LDS_SB = 64), 65 read them from global memory
@pytest.mark.parametrize("n,k", [(70001, 5), ((1 << 18) + 9, 6), (1100, 2), (300, 0)])
def test_wide_kmer_table_dna(n, k, dna70001):
    trio = dna70001 if n == 70001 else _Trio(W.dna_text_np(n, 11 + n), 4)
    assert trio.table.kmer_k() == k
    flat, off = W.ragged_patterns_np(4000, 24, 4, 5 + n)              # random: mostly absent k-mers, the early-exit pairs
    trio.check(flat, off)
    for m in sorted({max(k - 1, 1), max(k, 1), k + 1, 2 * k + 3}):
        flat2, off2, _ = W.substring_patterns_np(trio.text, 3000, m, 60 + m)   # present patterns
        trio.check(flat2, off2)
    if trio is not dna70001:
        trio.close()


# 2^(bits k) <= 10000 / 32 = 312: 2^8, 2^8 (k <= 16 does not bind), 4^4, 8^2.  At max_character 3 the codes that hold
# the unused value 3 (symbol 4) are never produced: such a symbol is out of range and the stepwise path reports it
@pytest.mark.parametrize("maxc,k", [(1, 8), (2, 8), (3, 4), (7, 2)])
def test_wide_kmer_table_other_one_level_alphabets(maxc, k):
    n = 10000
    t = ((W.splitmix64_np(maxc, 0, n) % np.uint64(maxc)) + np.uint64(1)).astype(np.uint8)
    t[-1] = 0
    trio = _Trio(t, maxc)
    assert trio.table.kmer_k() == k
    flat, off = W.ragged_patterns_np(3000, 30, maxc, 17)
    trio.check(flat, off)
    for m in (k, k + 5):
        flat2, off2, _ = W.substring_patterns_np(t, 2000, m, 3 + m)
        trio.check(flat2, off2)
    if maxc == 3:
        bad = flat.copy()
        bad[int(off[-1]) - 2] = 4                    # inside the last k symbols of the last non-empty pattern
        for g in (trio.table, trio.plain):
            with pytest.raises(F.Error) as ei:
                g.search_many(flat=bad, off=off)
            assert ei.value.code == F._lib.ERR_SYMBOL_RANGE
    trio.close()


def test_wide_kmer_table_zero_and_out_of_range_symbols_take_the_stepwise_path(dna70001):
    trio = dna70001
    k = trio.table.kmer_k()
    assert k == 5
    base, off, _ = W.substring_patterns_np(trio.text, 64, 20, 8)
    base = base.reshape(64, 20).copy()
    for r in range(64):
        base[r, 19 - (r % 10)] = 0                   # a zero inside / outside the last k symbols
    trio.check(base.reshape(-1), off)
    bad = base.copy()
    bad[bad == 0] = 6                                # > max_character, inside the last k symbols in half of the rows
    for g in (trio.table, trio.plain):
        with pytest.raises(F.Error) as ei:
            g.search_many(flat=bad.reshape(-1), off=off)
        assert ei.value.code == F._lib.ERR_SYMBOL_RANGE
    only_inside = bad[(np.arange(64) % 10) < k]      # ... and in every row
    off_in = np.arange(len(only_inside) + 1, dtype=np.uint64) * np.uint64(20)
    with pytest.raises(F.Error) as ei:
        trio.table.search_many(flat=only_inside.reshape(-1), off=off_in)
    assert ei.value.code == F._lib.ERR_SYMBOL_RANGE
    # the terminator row itself: "\0" alone, "x\0", "\0x"; and empty patterns next to long ones
    flat2, off2 = F.pack_patterns([bytes([0]), bytes([1, 0]), bytes([0, 1]), b"", bytes([1, 2, 3, 4, 1, 2, 3]), b""])
    trio.check(flat2, off2)
    flat3 = np.zeros(1, dtype=np.uint8)
    trio.check(flat3, np.zeros(9, dtype=np.uint64))  # eight empty patterns: (0, n)


def test_wide_kmer_table_refinement_ignores_the_table(dna70001):
    trio = dna70001
    flat, off, _ = W.substring_patterns_np(trio.text, 800, 5, 4)
    first = trio.plain.search_many(flat=flat, off=off)
    se = np.stack([first.s, first.e], axis=1).reshape(-1)
    flat2, off2 = W.ragged_patterns_np(800, 15, 4, 6)
    trio.check(flat2, off2, s0e0=se)


def _generic_text(kind, maxc, alphabet, n, repeat):
    t = ((W.splitmix64_np(maxc + n, 0, n) % np.uint64(alphabet)) + np.uint64(1)).astype(np.uint8)
    if repeat > 1:                                   # give the run-length index some runs
        t = np.repeat(t[: n // repeat + 1], repeat)[:n].copy()
    if kind == "multi":
        t[np.arange(997, n - 5, 4001)] = 0
    t[-1] = 0
    return t


# one 4-bit level: 16^2 <= 20000 / 32 = 625, 16^3 <= 4096; 5 superblocks keep their bases in LDS (FMXW_GLDS_SB = 8), 33 read
# them from global memory.  RLFM: 4^5 <= 60000 / 32 = 1875, 64^2 <= 140000 / 32 = 4375.  FM over two levels: ignored
@pytest.mark.parametrize("kind,maxc,alphabet,n,repeat,k", [
    ("fm", 15, 12, 20000, 1, 2), ("multi", 15, 12, 20000, 1, 2),
    ("fm", 15, 12, (1 << 17) + 5, 1, 3), ("multi", 15, 12, (1 << 17) + 5, 1, 3),
    ("rlfm", 4, 4, 60000, 4, 5), ("rlfm", 63, 50, 140000, 3, 2), ("fm", 63, 63, 140000, 1, 0)])
def test_wide_kmer_table_generic_kernels(kind, maxc, alphabet, n, repeat, k):
    t = _generic_text(kind, maxc, alphabet, n, repeat)
    trio = _Trio(t, maxc, kind=kind, narrow=n <= 60000)
    assert trio.table.kmer_k() == k
    kk = max(k, 2)
    flat, off = W.ragged_patterns_np(3000, 9, alphabet, 5 + maxc)
    trio.check(flat, off)
    for m in (kk - 1, kk, kk + 1, 2 * kk + 3):
        flat2, off2, _ = W.substring_patterns_np(t, 2000, m, 7 + m)
        trio.check(flat2, off2)
    flat3, off3 = F.pack_patterns([bytes([0]), bytes([1, 0]), bytes([0, 1]), b"", bytes([1, 2, 3, 0, 1, 2, 3, 4]),
                                   bytes([2, 2, 2, 2, 2, 2])])
    trio.check(flat3, off3)
    if kind == "multi":   # the start-of-piece / end-of-piece searches go through s0e0 or the row filter
        g, plain = trio.table, trio.plain
        for p in (bytes(t[998:1003]), bytes(t[5000:5004]), bytes(t[4990:4998]), bytes([2, 2, 2])):
            assert g.search_prefix(p).count() == plain.search_prefix(p).count()
            assert g.search_suffix(p).count() == plain.search_suffix(p).count()
            assert g.search_exact(p).count() == plain.search_exact(p).count()
            assert sorted(g.search_prefix(p).piece_ids()) == sorted(plain.search_prefix(p).piece_ids())
    trio.close()


def test_wide_kmer_table_wider_symbols_ignore_the_flag():
    t = W.dna_text_np(20000, 3).astype(np.uint16)
    g = F.FMIndex(F.Text.with_max_character(t, 4), kmer_table=True, force_wide=True)
    assert g.is_wide() and g.kmer_k() == 0
    flat, off, _ = W.substring_patterns_np(t, 500, 9, 2)
    os_, oe = O.OracleIndex(t.astype(np.uint8), 4).count_batch(flat.astype(np.uint8), off)
    _same(g.search_many(flat=flat.astype(np.uint16), off=off), os_, oe)
    g.close()


def _build_for_file(kind):
    n = 20001
    if kind == "fm":
        t = W.dna_text_np(n, 8)
        return t, F.FMIndexWithLocate(F.Text.with_max_character(t, 4), 2, kmer_table=True, force_wide=True), F.FMIndexWithLocate
    t = _generic_text("rlfm", 4, 4, n, 4)
    return t, F.RLFMIndexWithLocate(F.Text.with_max_character(t, 4), 2, kmer_table=True, force_wide=True), F.RLFMIndexWithLocate


@pytest.mark.parametrize("kind", ["fm", "rlfm"])
def test_wide_kmer_table_survives_save_load_and_damaged_files_are_refused(tmp_path, kind):
    t, g, cls = _build_for_file(kind)
    assert g.is_wide() and g.kmer_k() == 4           # 4^4 <= 20001 / 32 = 625
    flat, off = W.ragged_patterns_np(3000, 20, 4, 2)
    flat2, off2, _ = W.substring_patterns_np(t, 2000, 9, 4)
    path = str(tmp_path / "k.fmx")
    g.save(path)
    g2 = cls.load(path)
    assert g2.is_wide() and g2.kmer_k() == g.kmer_k() and g2.heap_size() == g.heap_size()
    oi = O.OracleIndex(t, 4, kind=kind)
    for fl, of in ((flat, off), (flat2, off2)):
        os_, oe = oi.count_batch(fl, of)
        _same(g.search_many(flat=fl, off=of), os_, oe)
        _same(g2.search_many(flat=fl, off=of), os_, oe)
    g2.close()
    oi.close()
    # damaged files: load and free only -- a handle loaded from a damaged file is never queried
    raw = bytearray(open(path, "rb").read())
    lib = g._lib
    hdr = 8 + 4 + 4 + 5 * 8 + 4 * 4
    dev_bytes = struct.unpack_from("<I", raw, 12)[0] & 0x7FFFFFFF      # (the top bit marks a wide file)
    assert 0 < dev_bytes < 4096 and hdr + dev_bytes < len(raw)

    def load(buf):
        p = str(tmp_path / "y.fmx")
        open(p, "wb").write(bytes(buf))
        h = C.c_void_p()
        rc = lib.fmx_load(p.encode(), 0, C.byref(h))
        if rc == 0:
            lib.fmx_free(h)
        return rc
    assert load(raw) == 0
    assert load(raw[:len(raw) // 2]) != 0            # truncated: inside the arrays
    assert load(raw[:len(raw) - 16]) != 0            # ... the last table entry is missing
    assert load(raw[:hdr + dev_bytes - 4]) != 0      # ... inside the device struct
    assert load(raw + bytes(16)) != 0                # trailing bytes
    refused = set()
    for o in range(hdr, hdr + dev_bytes, 4):
        for val in (0xFFFFFFFF, 200, 0x7FFFFFF0):
            bad = bytearray(raw)
            struct.pack_into("<I", bad, o, val)
            if bad == raw:
                continue
            if load(bad) != 0:
                refused.add((o - hdr, val))
    # the table's fields are the last of the struct: presence flag (8 bytes), kmer_k, kmer_bits
    for o in range(dev_bytes - 16, dev_bytes, 4):
        for val in (0xFFFFFFFF, 200, 0x7FFFFFF0):
            assert (o, val) in refused, (o, val)
    # a file without the table: setting the flag, k or bits alone is refused too (no blob behind the flag)
    g.close()
    t, g0, cls = _build_for_file(kind)
    g0.close()
    p0 = cls(F.Text.with_max_character(t, 4), 2, force_wide=True)
    assert p0.kmer_k() == 0
    p0.save(path)
    p0.close()
    raw0 = bytearray(open(path, "rb").read())
    assert load(raw0) == 0
    for o in range(dev_bytes - 16, dev_bytes, 4):
        for val in (1, 4, 200, 0xFFFFFFFF):
            bad = bytearray(raw0)
            struct.pack_into("<I", bad, hdr + o, val)
            assert load(bad) != 0, (o, val)


@pytest.mark.parametrize("kind", ["fm", "rlfm"])
def test_wide_kmer_table_replicas(kind):
    n = 50001
    t = W.dna_text_np(n, 17) if kind == "fm" else _generic_text("rlfm", 4, 4, n, 4)
    g = _CLS[kind](F.Text.with_max_character(t, 4), kmer_table=True, force_wide=True)
    assert g.is_wide() and g.kmer_k() == 5           # 4^5 <= 50001 / 32 = 1562
    reps = F.Replicas.of(g, [0, 0])
    assert [int(ix._lib.fmx_kmer_k(ix.handle())) for ix in reps.indexes] == [5, 5, 5]
    assert all(ix.heap_size() == g.heap_size() for ix in reps.indexes)
    flat, off = W.ragged_patterns_np(3001, 20, 4, 41)
    flat2, off2, _ = W.substring_patterns_np(t, 3001, 11, 43)
    oi = O.OracleIndex(t, 4, kind=kind)
    for fl, of in ((flat, off), (flat2, off2)):
        one = g.search_many(flat=fl, off=of)
        b = reps.search_many(flat=fl, off=of)
        assert (b.s == one.s).all() and (b.e == one.e).all() and (b.counts == one.counts).all()
        os_, oe = oi.count_batch(fl, of)
        _same(b, os_, oe)
    oi.close()
    reps.close()
