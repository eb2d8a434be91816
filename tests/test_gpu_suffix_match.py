"""Batched longest-suffix match (include/fmx.h: fmx_suffix_match_batch / _dev / _multi) against the loop of the header run
over the CPU oracle (tests/suffix_match_expect.py), through the C ABI: every index kind, both engines, the k-mer table
and pair-index shortcuts, min_count 1 / 2 / 5, refinement from a previous result, and the argument checks."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import fm_index_amd as F
from fm_index_amd import _lib as L
from fm_index_amd import workload as W
from oracle import fm_oracle as O
from suffix_match_expect import expect_suffix_match

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 5, 255, 256, 257, 1000, 20001]


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def abi_match(gi, flat, off, s0e0=None, min_count=1, want=(True, True, True, True)):
    """fmx_suffix_match_batch on host arrays: (rc, s, e, count, len); an output that is not wanted is passed as NULL"""
    flat = np.ascontiguousarray(flat, dtype=gi._dtype)
    off = np.ascontiguousarray(off, dtype=np.uint64)
    npat = len(off) - 1
    outs = [np.full(max(npat, 1), 0xDEAD, dtype=np.uint64) if w else None for w in want]
    se = None if s0e0 is None else np.ascontiguousarray(s0e0, dtype=np.uint64)
    rc = gi._lib.fmx_suffix_match_batch(gi.handle(), _ptr(flat), _ptr(off), npat, _ptr(se), int(min_count),
                                        *[_ptr(o) for o in outs])
    return (rc,) + tuple(None if o is None else o[:npat] for o in outs)


def abi_count(gi, flat, off):
    flat = np.ascontiguousarray(flat, dtype=gi._dtype)
    off = np.ascontiguousarray(off, dtype=np.uint64)
    npat = len(off) - 1
    s, e, c = (np.zeros(max(npat, 1), dtype=np.uint64) for _ in range(3))
    rc = gi._lib.fmx_count_batch(gi.handle(), _ptr(flat), _ptr(off), npat, None, _ptr(s), _ptr(e), _ptr(c))
    return rc, s[:npat], e[:npat], c[:npat]


def pack(pats, dtype):
    off = np.zeros(len(pats) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(p) for p in pats], dtype=np.uint64)
    flat = np.concatenate([np.asarray(p, dtype=dtype) for p in pats] + [np.zeros(1, dtype=dtype)])
    return flat, off


def make_batch(t, maxc, rng, per=80, mmax=40):
    """the pattern mix: `per` substrings, `per` substrings with one symbol changed at a uniform position, and `per` others
    -- random patterns, patterns with a 0, patterns with a symbol above max_character (within the last 12 symbols, so
    that every short matched length occurs); lengths 0..mmax.  Returns (patterns, index of the first out-of-range one
    or None)"""
    n, dt = len(t), t.dtype
    hi = maxc + 1 if maxc + 1 <= int(np.iinfo(dt).max) else None

    def sub(mmin=0):
        m = int(rng.integers(mmin, max(min(mmax, n - 1), mmin) + 1))
        if m > n - 1:
            return rng.integers(1, maxc + 1, m).astype(dt)
        a = int(rng.integers(0, n - m))
        return t[a:a + m].copy()

    pats = [sub() for _ in range(per)]
    for _ in range(per):
        p = sub(1)
        p[int(rng.integers(0, len(p)))] = rng.integers(1, maxc + 1)
        pats.append(p)
    first_hi = None
    for q in range(per):
        if q % 3 == 0:
            pats.append(rng.integers(1, maxc + 1, int(rng.integers(0, mmax + 1))).astype(dt))
        elif q % 3 == 1 or hi is None:
            p = sub(1)
            p[int(rng.integers(0, len(p)))] = 0
            pats.append(p)
        else:
            p = sub(1)
            p[len(p) - 1 - int(rng.integers(0, min(len(p), 12)))] = hi
            first_hi = len(pats) if first_hi is None else first_hi
            pats.append(p)
    if hi is not None and n > 24:      # ... and one substring per short length whose match must end after exactly j symbols
        for j in range(9):
            p = sub(20)[:20]
            p[len(p) - 1 - j] = hi
            pats.append(p)
    return pats, first_hi


def check_index(gi, oi, t, maxc, seed, need=()):
    """every min_count, then a refinement batch from the first result; returns the set of matched lengths seen"""
    rng = np.random.default_rng(seed)
    pats, first_hi = make_batch(t, maxc, rng)
    flat, off = pack(pats, t.dtype)
    seen = set()
    first = None
    for mc in (1, 2, 5):
        rc, s, e, c, ln = abi_match(gi, flat, off, min_count=mc)
        assert rc == L.OK, (rc, gi._lib.fmx_last_error())              # out-of-range symbols are no error here
        ws, we, wc, wl = expect_suffix_match(oi, flat, off, min_count=mc)
        bad = np.nonzero((s != ws) | (e != we) | (c != wc) | (ln != wl))[0]
        assert len(bad) == 0, (len(t), mc, int(bad[0]), pats[int(bad[0])].tolist(),
                               (int(s[bad[0]]), int(e[bad[0]]), int(ln[bad[0]])),
                               (int(ws[bad[0]]), int(we[bad[0]]), int(wl[bad[0]])))
        seen |= set(int(x) for x in ln)
        first = (s, e) if first is None else first
    if first_hi is not None and len(t) >= 255:     # ... and fmx_count_batch does report them (true substrings reach them)
        assert abi_count(gi, flat, off)[0] == L.ERR_SYMBOL_RANGE
    # refinement: the patterns rotated by one against the intervals of the first result
    se = np.stack([np.roll(first[0], 1), np.roll(first[1], 1)], axis=1).reshape(-1)
    for mc in (1, 2):
        rc, s, e, c, ln = abi_match(gi, flat, off, s0e0=se, min_count=mc)
        assert rc == L.OK
        ws, we, wc, wl = expect_suffix_match(oi, flat, off, s0e0=se, min_count=mc)
        assert (s == ws).all() and (e == we).all() and (c == wc).all() and (ln == wl).all(), (len(t), mc)
    assert set(need) <= seen, (sorted(set(need) - seen), sorted(seen))
    return seen


def dna(n, seed):
    t = (W.splitmix64_np(seed, 0, n) % np.uint64(4)).astype(np.uint8) + 1
    t[-1] = 0
    return t


def sym_text(n, seed, sigma, dtype=np.uint8):
    t = ((W.splitmix64_np(seed, 0, n) % np.uint64(sigma)) + np.uint64(1)).astype(dtype)
    t[-1] = 0
    return t


def run_text(n, seed, runlen=64):
    base = ((W.splitmix64_np(seed, 0, n // runlen + 2) % np.uint64(5)) + np.uint64(1)).astype(np.uint8)
    t = np.repeat(base, runlen)[:n].copy()
    t[-1] = 0
    return t


def pieces_text(n, seed):
    t = sym_text(n, seed, 200)
    t[37::53] = 0                                          # several pieces, no two end markers in a row
    t[-1] = 0
    if n > 1 and t[-2] == 0:
        t[-2] = 1
    return t


DNA_KW = {"plain": dict(plain=True), "pair": dict(pair_index=True), "kmer": dict(kmer_table=True),
          "both": dict(pair_index=True, kmer_table=True), "auto": dict(auto=True)}


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("variant", list(DNA_KW))
def test_dna_every_accelerator(variant, wide):
    """FM over sigma = 4: plain, pair index, k-mer table, both, and the builder's own choice; n up to 70001 so that
    k >= 5.  From n = 20001 on (where the table exists and the text holds every short k-mer) the batch must show L = 0,
    1, k-1, k, k+1 and both parities of the pair step."""
    for n in SIZES + [70001]:
        if wide and n < 2:
            continue
        t = dna(n, 100 + n)
        gi = F.FMIndexWithLocate(F.Text.with_max_character(t, 4), 2, force_wide=wide, **DNA_KW[variant])
        assert gi.is_wide() == wide
        if variant in ("pair", "both"):
            assert gi.has_pair_index() == (n >= 4)         # (the builder makes none for texts below four symbols)
        k = gi.kmer_k()
        if variant in ("kmer", "both") and n >= 20001:
            assert k >= (5 if n == 70001 else 2)
        need = ()
        if n >= 20001:
            kk = k if k else 4
            need = {0, 1, 2, 3, kk - 1, kk, kk + 1}
        oi = O.OracleIndex(t, 4)
        check_index(gi, oi, t, 4, 7 * n + wide, need)
        gi.close()


def vocab_text(n, seed):
    """a sigma = 4 text made of eight 16-symbol words: at most 8 * 16 + 64 * (k - 1) of the 4^k k-mers occur, so most
    entries of a k-mer table (k >= 4) are empty and many of the others hold a handful of rows"""
    rng = np.random.default_rng(seed)
    words = rng.integers(1, 5, (8, 16)).astype(np.uint8)
    t = words[rng.integers(0, 8, n // 16 + 1)].reshape(-1)[:n].copy()
    t[-1] = 0
    return t


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("variant", ["kmer", "both", "auto"])
def test_kmer_table_entry_below_min_count_restarts_stepwise(variant, wide):
    """the table's miss branch: a pattern of k symbols or more, all of its last k in 1..4, whose table entry holds
    fewer than min_count rows must come back with the stepwise answer from (0, len) -- L < k.  The batch must hold
    such patterns (asserted wherever the index has a table of k >= 3) at every min_count."""
    for n in (1000, 20001, 70001):
        t = vocab_text(n, 900 + n)
        gi = F.FMIndexWithLocate(F.Text.with_max_character(t, 4), 2, force_wide=wide, **DNA_KW[variant])
        oi = O.OracleIndex(t, 4)
        k = gi.kmer_k()
        if variant != "auto" and n >= 20001:
            assert k >= 3
        pats, _ = make_batch(t, 4, np.random.default_rng(31 * n + wide), per=120)
        flat, off = pack(pats, np.uint8)
        asks = np.array([k > 0 and len(p) >= k and int(p[len(p) - k:].min()) >= 1 and int(p[len(p) - k:].max()) <= 4
                         for p in pats])                                # patterns that look their start up in the table
        for mc in (1, 2, 5):
            rc, s, e, c, ln = abi_match(gi, flat, off, min_count=mc)
            assert rc == L.OK
            ws, we, wc, wl = expect_suffix_match(oi, flat, off, min_count=mc)
            assert (s == ws).all() and (e == we).all() and (c == wc).all() and (ln == wl).all(), (n, mc, k)
            if k >= 3:
                missed = asks & (ln < k)
                assert int(missed.sum()) >= 10, (n, mc, k, int(missed.sum()))
                assert int((asks & (ln >= k)).sum()) >= 10               # ... next to patterns whose entry is taken
        gi.close()


def test_start_pair_with_e_below_s_holds_no_row():
    """a given (s, e) with e < s: L = 0, the pair comes back, out_count = 0 -- on the group-per-pattern and the
    endpoint-per-lane kernels of both engines"""
    n = 20001
    td, tr = dna(n, 41), run_text(n, 42)
    for wide in (False, True):
        for gi, oi, t, maxc in (
                (F.FMIndexWithLocate(F.Text.with_max_character(td, 4), 2, force_wide=wide, kmer_table=True,
                                     pair_index=True), O.OracleIndex(td, 4), td, 4),
                (F.FMIndexWithLocate(F.Text.with_max_character(td, 4), 2, force_wide=wide, plain=True),
                 O.OracleIndex(td, 4), td, 4),
                (F.RLFMIndexWithLocate(F.Text.with_max_character(tr, 5), 2, force_wide=wide),
                 O.OracleIndex(tr, 5, kind="rlfm"), tr, 5)):
            pats = [t[100:100 + m].copy() for m in (0, 1, 7, 20, 20, 3)]
            flat, off = pack(pats, np.uint8)
            se = np.array([5, 3, n, 0, 0, n, 9, 2, 0, n, 7, 7], dtype=np.uint64)
            for mc in (1, 3):
                rc, s, e, c, ln = abi_match(gi, flat, off, s0e0=se, min_count=mc)
                assert rc == L.OK
                ws, we, wc, wl = expect_suffix_match(oi, flat, off, s0e0=se, min_count=mc)
                assert (s == ws).all() and (e == we).all() and (c == wc).all() and (ln == wl).all()
                for q in (0, 1, 3):
                    assert (int(s[q]), int(e[q]), int(c[q]), int(ln[q])) == (int(se[2 * q]), int(se[2 * q + 1]), 0, 0)
            gi.close()


_FORCED = r"""
import sys
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import numpy as np
import fm_index_amd as F
from fm_index_amd import _lib as L
from oracle import fm_oracle as O
import test_gpu_suffix_match as T
assert L.LIB_PATH.endswith("libfmx_measure.so")
n = 20001
cases = []
for wide in (False, True):
    t = T.sym_text(n, 71, 200)
    cases.append((F.RLFMIndexWithLocate(F.Text.with_max_character(t, 200), 2, force_wide=wide),
                  O.OracleIndex(t, 200, kind="rlfm"), t, 200))
    t = T.run_text(n, 72)
    cases.append((F.RLFMIndexWithLocate(F.Text.with_max_character(t, 5), 2, force_wide=wide),
                  O.OracleIndex(t, 5, kind="rlfm"), t, 5))
    t = T.sym_text(n, 73, 200)
    cases.append((F.FMIndexWithLocate(F.Text.with_max_character(t, 200), 2, force_wide=wide),
                  O.OracleIndex(t, 200), t, 200))
    t = T.pieces_text(n, 74)
    cases.append((F.FMIndexMultiPiecesWithLocate(F.Text.with_max_character(t, 200), 2, force_wide=wide),
                  O.OracleIndex(t, 200, kind="multi"), t, 200))
for q, (gi, oi, t, maxc) in enumerate(cases):
    T.check_index(gi, oi, t, maxc, 50 + q)
    gi.close()
print("forced ok", len(cases))
"""


def test_group_per_pattern_twins_through_the_measurement_build():
    """the twins the shipped dispatch never picks for indexes the builder makes -- fmx_sfx_kernel on a run-length index
    (hints + record search, SM = 0) and fmxw_g_sfx_kernel on every generic wide index -- forced by the measurement
    build's switches (FMX_VARIANT=0, FMXW_R_COUNT_GROUP=1) in a process of its own: the oracle's answers"""
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = os.path.join(root, "fm_index_amd", "libfmx_measure.so")
    assert os.path.exists(lib), "fm_index_amd/libfmx_measure.so is missing: run `make -C fm_index_amd/csrc measure`"
    p = subprocess.run([sys.executable, "-c", _FORCED % (root, os.path.join(root, "tests"))],
                       env=dict(os.environ, FMX_LIB=lib, FMX_VARIANT="0", FMXW_R_COUNT_GROUP="1"),
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert p.returncode == 0, p.stderr.decode(errors="replace")[-3000:]
    assert b"forced ok 8" in p.stdout


@pytest.mark.parametrize("wide", [False, True])
def test_fm_bytes_two_levels(wide):
    for n in SIZES:
        if wide and n < 2:
            continue
        t = sym_text(n, 200 + n, 200)
        gi = F.FMIndexWithLocate(F.Text.with_max_character(t, 200), 2, force_wide=wide)
        check_index(gi, O.OracleIndex(t, 200), t, 200, 11 * n + wide)
        gi.close()


@pytest.mark.parametrize("wide", [False, True])
def test_fm_u16_symbols(wide):
    for n in SIZES:
        if wide and n < 2:
            continue
        t = sym_text(n, 300 + n, 1000, np.uint16)
        gi = F.FMIndexWithLocate(F.Text.with_max_character(t, 1000), 2, force_wide=wide)
        assert gi._dtype == np.uint16
        check_index(gi, O.OracleIndex(t, 1000), t, 1000, 13 * n + wide)
        gi.close()


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("text", ["random", "runs"])
def test_rlfm_both_select_structures(text, wide):
    """random text: select blocks; long runs: stored positions -- the two structures the builder makes (an index of
    these sizes never gets the hints + record search of the generic kernel)"""
    for n in SIZES[1:]:
        t = sym_text(n, 400 + n, 200) if text == "random" else run_text(n, 500 + n)
        maxc = 200 if text == "random" else 5
        gi = F.RLFMIndexWithLocate(F.Text.with_max_character(t, maxc), 2, force_wide=wide)
        check_index(gi, O.OracleIndex(t, maxc, kind="rlfm"), t, maxc, 17 * n + wide)
        gi.close()


@pytest.mark.parametrize("wide", [False, True])
def test_multi_pieces(wide):
    for n in SIZES:
        if wide and n < 2:
            continue
        t = pieces_text(n, 600 + n)
        gi = F.FMIndexMultiPiecesWithLocate(F.Text.with_max_character(t, 200), 2, force_wide=wide)
        check_index(gi, O.OracleIndex(t, 200, kind="multi"), t, 200, 19 * n + wide)
        gi.close()


def test_empty_text():
    """n = 0: the start pair (0, 0) is below every min_count -- L = 0 and (0, 0), whatever the pattern holds"""
    for cls in (F.FMIndex, F.RLFMIndex):
        try:
            gi = cls(F.Text(b""))
        except F.Error as ex:                              # (the run-length index refuses texts below two symbols)
            assert cls is F.RLFMIndex and ex.code == L.ERR_UNSUPPORTED
            continue
        flat, off = pack([np.array(p, dtype=np.uint8) for p in ([1], [], [1, 2], [0], [255, 3])], np.uint8)
        for mc in (0, 1, 5):
            rc, s, e, c, ln = abi_match(gi, flat, off, min_count=mc)
            assert rc == L.OK and not s.any() and not e.any() and not c.any() and not ln.any()
        rc = abi_match(gi, flat, off, s0e0=np.array([0, 0] * 4 + [0, 1], dtype=np.uint64))[0]
        assert rc == L.ERR_ARG
        gi.close()


def test_self_consistency_default_index_2_20():
    """no oracle: on n = 2^20 DNA with the default index, fmx_count_batch of each pattern's last L symbols gives the same
    (s, e), and of its last L + 1 symbols (where L < m) fewer than min_count rows"""
    n = 1 << 20
    t = W.dna_text_np(n, 9)
    gi = F.FMIndexWithLocate(F.Text.with_max_character(t, 4), 2)
    rng = np.random.default_rng(5)
    pats = []
    for q in range(3000):
        m = int(rng.integers(0, 41))
        a = int(rng.integers(0, n - 1 - m))
        p = t[a:a + m].copy()
        if m and q % 3:
            p[int(rng.integers(0, m))] = rng.integers(1, 5)
        pats.append(p)
    flat, off = pack(pats, np.uint8)
    for mc in (1, 2, 5):
        rc, s, e, c, ln = abi_match(gi, flat, off, min_count=mc)
        assert rc == L.OK and (c == e - s).all() and (c >= mc).all()
        f1, o1 = pack([p[len(p) - int(l):] for p, l in zip(pats, ln)], np.uint8)
        rc, cs, ce, _ = abi_count(gi, f1, o1)
        assert rc == L.OK and (cs == s).all() and (ce == e).all()
        longer = [k for k, p in enumerate(pats) if int(ln[k]) < len(p)]
        assert longer
        f2, o2 = pack([pats[k][len(pats[k]) - int(ln[k]) - 1:] for k in longer], np.uint8)
        rc, _, _, cc = abi_count(gi, f2, o2)
        assert rc == L.OK and (cc < mc).all()
    gi.close()


def test_dev_form_on_a_stream_with_null_outputs_and_errors():
    """the _dev form on a non-default stream, out_s / out_e NULL; bad offsets and an s0e0 entry above len() are
    FMX_ERR_ARG on both forms (outputs of such a pattern 0), reported by the _dev form through fmx_stream_status"""
    import torch
    n = 20001
    t = dna(n, 77)
    gi = F.FMIndexWithLocate(F.Text.with_max_character(t, 4), 2, kmer_table=True)
    oi = O.OracleIndex(t, 4)
    pats, _ = make_batch(t, 4, np.random.default_rng(3))
    flat, off = pack(pats, np.uint8)
    npat = len(pats)
    ws, we, wc, wl = expect_suffix_match(oi, flat, off, min_count=2)
    lib = gi._lib
    st = torch.cuda.Stream()
    d_flat = torch.from_numpy(flat).cuda()
    d_off = torch.from_numpy(off.astype(np.int64)).cuda()
    d_c = torch.zeros(npat, dtype=torch.int64, device="cuda")
    d_l = torch.zeros(npat, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    rc = lib.fmx_suffix_match_batch_dev(gi.handle(), d_flat.data_ptr(), d_off.data_ptr(), npat, None, 2, None, None,
                                        d_c.data_ptr(), d_l.data_ptr(), st.cuda_stream)
    assert rc == L.OK
    st.synchronize()
    assert lib.fmx_stream_status(gi.handle()) == L.OK
    assert (d_c.cpu().numpy().astype(np.uint64) == wc).all() and (d_l.cpu().numpy().astype(np.uint64) == wl).all()
    # host form: only out_len, then only out_s
    rc, s, e, c, ln = abi_match(gi, flat, off, min_count=2, want=(False, False, False, True))
    assert rc == L.OK and s is None and (ln == wl).all()
    rc, s, e, c, ln = abi_match(gi, flat, off, min_count=2, want=(True, False, False, False))
    assert rc == L.OK and (s == ws).all()
    # offsets that go backwards (pattern 1), an s0e0 entry above len() (pattern 2)
    boff = off.copy()
    kb = int(np.nonzero(off >= 1)[0][0])                               # pattern kb ends before it begins
    boff[kb + 1] = off[kb] - np.uint64(1)
    rc, s, e, c, ln = abi_match(gi, flat, boff, min_count=2)
    assert rc == L.ERR_ARG and s[kb] == 0 and e[kb] == 0 and c[kb] == 0 and ln[kb] == 0
    assert (ln[kb + 2:] == wl[kb + 2:]).all() and (s[kb + 2:] == ws[kb + 2:]).all() and (ln[:kb] == wl[:kb]).all()
    se = np.tile(np.array([0, n], dtype=np.uint64), npat)
    se[5] = n + 1
    rc, s, e, c, ln = abi_match(gi, flat, off, s0e0=se, min_count=2)
    assert rc == L.ERR_ARG and s[2] == 0 and e[2] == 0 and ln[2] == 0
    keep = np.arange(npat) != 2
    assert (ln[keep] == wl[keep]).all() and (e[keep] == we[keep]).all()
    for d_bad_off, d_bad_se in ((torch.from_numpy(boff.astype(np.int64)).cuda(), None),
                                (d_off, torch.from_numpy(se.astype(np.int64)).cuda())):
        torch.cuda.synchronize()
        rc = lib.fmx_suffix_match_batch_dev(gi.handle(), d_flat.data_ptr(), d_bad_off.data_ptr(), npat,
                                            None if d_bad_se is None else d_bad_se.data_ptr(), 2, None, None,
                                            d_c.data_ptr(), d_l.data_ptr(), st.cuda_stream)
        assert rc == L.OK
        st.synchronize()
        assert lib.fmx_stream_status(gi.handle()) == L.ERR_ARG
        assert lib.fmx_stream_status(gi.handle()) == L.OK              # reading cleared it
    gi.close()


@pytest.mark.parametrize("g", [1, 2, 3])
def test_multi_over_replicas_equals_one_handle(g):
    n = 20001
    t = dna(n, 88)
    gi = F.FMIndexWithLocate(F.Text.with_max_character(t, 4), 2, pair_index=True)
    reps = F.Replicas.of(gi, [0] * (g - 1))
    assert len(reps) == g
    pats, _ = make_batch(t, 4, np.random.default_rng(g), per=67)       # 201 patterns: ragged shards at g = 2
    flat, off = pack(pats, np.uint8)
    one = gi.suffix_match_many(flat=flat, off=off, min_count=2)
    many = reps.suffix_match_many(flat=flat, off=off, min_count=2)
    assert (one.s == many.s).all() and (one.e == many.e).all() and (one.counts == many.counts).all()
    assert (one.lengths == many.lengths).all() and one.lengths.dtype == np.uint64
    ws, we, wc, wl = expect_suffix_match(O.OracleIndex(t, 4), flat, off, min_count=2)
    assert (many.s == ws).all() and (many.e == we).all() and (many.lengths == wl).all()
    reps.close(keep_first=True)
    gi.close()


@pytest.mark.parametrize("kind", ["dna", "rlfm"])
def test_more_patterns_than_groups(kind):
    """a batch in which every group (2048 blocks x 32) and every lane pair of the endpoint kernel (1024 x 128) takes
    more than one pattern, on a small index (n = 2^16, as tests/test_gpu_large_batches.py)"""
    n = 1 << 16
    if kind == "dna":
        t = dna(n, 61)
        gi, oi, maxc = F.FMIndexWithLocate(F.Text.with_max_character(t, 4), 2), O.OracleIndex(t, 4), 4
    else:
        t = W.repetitive_text_np(n, 7, base_len=1 << 9, mut_per_1024=20)
        gi, oi, maxc = F.RLFMIndexWithLocate(F.Text(t), 2), O.OracleIndex(t, 255, kind="rlfm"), 255
    npat, m = 150000, 12
    rng = np.random.default_rng(12)
    a = rng.integers(0, n - 1 - m, npat)
    mat = t[a[:, None] + np.arange(m)[None, :]].copy()
    hit = rng.integers(0, 3, npat) > 0                                 # two thirds get one symbol changed
    mat[np.nonzero(hit)[0], rng.integers(0, m, int(hit.sum()))] = rng.integers(1, maxc + 1, int(hit.sum()))
    flat = np.ascontiguousarray(mat.reshape(-1))
    off = np.arange(npat + 1, dtype=np.uint64) * np.uint64(m)
    rc, s, e, c, ln = abi_match(gi, flat, off, min_count=2)
    assert rc == L.OK
    ws, we, wc, wl = expect_suffix_match(oi, flat, off, min_count=2)
    assert (s == ws).all() and (e == we).all() and (c == wc).all() and (ln == wl).all()
    gi.close()


def test_locate_gives_the_seed_positions():
    n = 20001
    t = dna(n, 99)
    gi = F.FMIndexWithLocate(F.Text.with_max_character(t, 4), 2)
    pats, _ = make_batch(t, 4, np.random.default_rng(8), per=40)
    pats = [p for p in pats if len(p) and int(p.max()) <= 4 and int(p.min()) >= 1]
    b = gi.suffix_match_many(patterns=pats, min_count=1)
    assert isinstance(b, F.SearchBatch) and len(b.lengths) == len(pats)
    hoff, pos = b.locate()
    assert int(hoff[-1]) == int(b.counts.sum())
    for k, p in enumerate(pats):
        ln = int(b.lengths[k])
        mine = pos[int(hoff[k]):int(hoff[k + 1])]
        assert len(mine) == int(b.counts[k]) >= 1
        if ln == 0:
            continue
        for q in mine[:50]:
            assert (t[int(q):int(q) + ln] == p[len(p) - ln:]).all(), (k, int(q), ln)
        assert len(mine) == len(O.naive_search(t, p[len(p) - ln:]))
        if ln < len(p):
            assert len(O.naive_search(t, p[len(p) - ln - 1:])) == 0
    gi.close()


CPP = r"""
#include <cstdio>
#include <cstring>
#include <string>
#include "fm_index.hpp"
int main() {
  try {
    const std::string s = "mississippi";
    std::vector<uint8_t> bytes(s.begin(), s.end());
    bytes.push_back(0);
    fmx::FMIndexWithLocate index(fmx::Text(bytes), 2);
    std::vector<std::vector<uint8_t>> pats;
    for (const char *w : {"pssi", "ssi", "x", ""}) pats.emplace_back(w, w + std::strlen(w));
    std::vector<uint64_t> a, b, l;
    for (uint64_t mc : {1, 3}) {
      index.suffix_match_many(pats, mc, a, b, l);
      for (size_t k = 0; k < pats.size(); k++)
        std::printf("%llu %llu %llu\n", (unsigned long long)a[k], (unsigned long long)b[k], (unsigned long long)l[k]);
    }
  } catch (const fmx::Error &e) {
    std::printf("FAILED %d %s\n", e.code, e.what());
    return 1;
  }
  return 0;
}
"""


def test_cpp_mirror(tmp_path):
    """fmx::Index::suffix_match_many (fm_index.hpp) on `mississippi`: the hand-worked answers of the CPU test"""
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "sfx.cpp"
    src.write_text(CPP)
    exe = str(tmp_path / "sfx")
    subprocess.check_call(["g++", "-std=c++17", "-I" + os.path.join(root, "include"),
                           "-I" + os.path.join(root, "fm_index_amd", "host"), str(src), "-o", exe,
                           "-L" + os.path.dirname(L.LIB_PATH), "-lfmx", "-Wl,-rpath," + os.path.dirname(L.LIB_PATH)])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.split("\n")[:8] == ["10 12 3", "10 12 3", "0 12 0", "0 12 0",
                                          "1 5 1", "1 5 1", "0 12 0", "0 12 0"]
