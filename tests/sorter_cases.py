"""Texts that take each exit of the GPU builder's prefix doubling (suffix_sort / suffix_sort_wide in
fm_index_amd/csrc/fmx_build.hip), and a plain numpy model of which exit a text takes.  Needs no GPU.

The exits, by the counts the sorters branch on (k = symbols per packed key, m = suffixes tied after the first round,
m2 = suffixes still tied at depth 2k, active(h) = suffixes tied after the full round at depth h):
  1  m == 0
  2  0 < 8 m <= n and m2 == 0: the text round (k_text_round_* / kwt_*) resolves every tie
  3  0 < 8 m <= n and m2 > 0: the text round hands over to refine() at depth 2k
  4  8 m > n: full rounds until 4 active(H) <= n at a depth H with 4 H < n, then refine() on the compacted list
  5  8 m > n and the full rounds go on to a depth H with 4 H >= n: all but the last two of the doublings a text of n
     symbols can need are full rounds (all-equal and periodic texts; refine() is left a handful of suffixes, or none)
Used by tests/test_sorter_cases_cpu.py, tests/sorter_branches.py and tests/test_gpu_sorter_branches.py."""
import collections

import numpy as np

from fm_index_amd import workload as W

SMALL_SIZES = (257, 4099, (1 << 17) + 5)          # 4099: inside the pooled scratch (kArenaMaxN = 2^17), the last: just above
THRESHOLD_SIZES = ((1 << 19) - 1, 1 << 19)        # kRefineMinN of the shipped 32-bit library, from both sides
THRESHOLD_CASES = ("short-copies", "long-copies", "tiled-block", "zero-runs")
ENGINES = ("32-bit", "wide")

Case = collections.namedtuple("Case", "name n text max_character kind branch")


def sym_bits(max_character):
    """the builders' sym_bits: 32 - clz(max_character) = floor(log2(max_character)) + 1"""
    return int(max_character).bit_length()


def key_symbols(max_character, engine):
    """symbols per packed key: min(32, 64 / bits) in suffix_sort, min(32, 63 / bits) in suffix_sort_wide"""
    return min(32, (63 if engine == "wide" else 64) // sym_bits(max_character))


def _packed(a, bits, k):
    """keys[i] = a[i .. i + k) packed `bits` bits each, for every i with i + k <= len(a)"""
    cnt = len(a) - k + 1
    key = np.zeros(cnt, dtype=np.uint64)
    for j in range(k):
        key = (key << np.uint64(bits)) | a[j:j + cnt]
    return key


def _tied(keys):
    """how many entries of `keys` equal another entry"""
    _, inv, cnt = np.unique(keys, return_inverse=True, return_counts=True)
    return int((cnt[inv.reshape(-1)] > 1).sum())


def tied_counts(t, bits, k):
    """(m, m2): the suffixes whose first k (2k) symbols, zero-padded past the end as pack_key does, equal another's"""
    n = len(t)
    a = np.concatenate([np.asarray(t, dtype=np.uint64), np.zeros(2 * k, dtype=np.uint64)])
    keys = _packed(a, bits, k)                    # n + k + 1 of them
    first, second = keys[:n], keys[k:k + n]
    m = _tied(first)
    g1 = np.unique(first, return_inverse=True)[1].reshape(-1).astype(np.uint64)
    g2 = np.unique(second, return_inverse=True)[1].reshape(-1).astype(np.uint64)
    return m, _tied(g1 * np.uint64(n) + g2)


def doubling_actives(t, bits, k):
    """[(h, active(h))] for h = k, 2k, 4k, ... down to the first active(h) == 0: the first round by the packed key, every
    later one by (group of i, group of i + h, or `ended` when i + h >= n), as k_double_keys / kw_key_second build them"""
    n = len(t)
    a = np.concatenate([np.asarray(t, dtype=np.uint64), np.zeros(k, dtype=np.uint64)])
    ids = np.unique(_packed(a, bits, k)[:n], return_inverse=True)[1].reshape(-1).astype(np.int64)
    out, h = [], k
    while True:
        act = int((np.bincount(ids)[ids] > 1).sum())
        out.append((h, act))
        if act == 0:
            return out
        nxt = np.zeros(n, dtype=np.int64)
        if h < n:
            nxt[:n - h] = ids[h:] + 1
        ids = np.unique(ids * (n + 1) + nxt, return_inverse=True)[1].reshape(-1).astype(np.int64)
        h *= 2


Prediction = collections.namedtuple("Prediction", "branch k m m2 depth actives refines")


def predict(case, engine):
    """the exit `case` takes on `engine` (refinement rounds enabled) and the counts its trace must show: `actives` are the
    (h, count) of the full rounds up to the hand-over at `depth`, `refines` the rounds refine() needs after them
    (branches 4 and 5)"""
    n = len(case.text)
    bits = sym_bits(case.max_character)
    k = key_symbols(case.max_character, engine)
    m, m2 = tied_counts(case.text, bits, k)
    if m == 0:
        return Prediction(1, k, 0, 0, k, [], 0)
    if 8 * m <= n:
        return Prediction(2 if m2 == 0 else 3, k, m, m2, 2 * k, [], None)
    act = doubling_actives(case.text, bits, k)
    stop = next(j for j, (_, a) in enumerate(act) if 4 * a <= n)
    big_h = act[stop][0]
    shown = act[:stop + 1] if act[stop][1] else act[:stop]       # (the round that leaves nothing tied prints no count)
    return Prediction(5 if 4 * big_h >= n else 4, k, m, m2, big_h, shown, len(act) - 1 - stop)


# ---- the texts ----------------------------------------------------------------------------------------------------
def _rnd(seed, count):
    return W.splitmix64_np(seed, 0, count)


def _random_text(n, seed, alphabet, dtype=np.uint8):
    t = (_rnd(seed, n) % np.uint64(alphabet)).astype(dtype) + 1
    t[n - 1] = 0
    return t


def _plant(t, src, dst, length, alphabet):
    """t[dst .. dst + length) becomes a copy of t[src .. src + length) that ends there: the next symbols differ"""
    assert src + length < dst and dst + length < len(t) - 1
    t[dst:dst + length] = t[src:src + length]
    if t[dst + length] == t[src + length]:
        t[dst + length] = t[src + length] % alphabet + 1


def _plant_all(t, lengths, alphabet, gap=16):
    src, dst = 1, len(t) // 2
    for length in lengths:
        _plant(t, src, dst, length, alphabet)
        src += length + gap
        dst += length + gap
    assert src < len(t) // 2
    return t


def _fib_word(n):
    a, b = b"\x01", b"\x01\x02"
    while len(b) < n:
        a, b = b, b + a
    return np.frombuffer(b[:n], dtype=np.uint8).copy()


def _unique(n):
    return _random_text(n, 101, 255), 255


def _short_copies(n):
    k = key_symbols(4, "32-bit")
    return _plant_all(_random_text(n, 102, 4), [k + 3] * min(50, n // 128), 4), 4


def _long_copies(n):
    k = key_symbols(4, "32-bit")
    if n < 16 * (2 * k + 5):          # one plant of 2k + 5 symbols ties 2 (k + 6) suffixes: more than n / 8
        return None
    return _plant_all(_random_text(n, 103, 4), [2 * k + 5, 5 * k, min(40 * k, n // 32)], 4), 4


def _copy_of_the_tail(n):
    k = key_symbols(4, "32-bit")
    length = 2 * k + 5
    if n < 16 * length:
        return None
    t = _random_text(n, 104, 4)
    t[n // 2:n // 2 + length] = t[n - 1 - length:n - 1]     # the original is followed by the terminator, the copy is not
    return t, 4


def _zero_runs(n):
    k = key_symbols(255, "32-bit")
    t = _random_text(n, 105, 255)
    for j, length in enumerate((1, k, k + 1, 2 * k, 2 * k + 3)):
        p = (j + 1) * n // 7
        t[p:p + length] = 0
    return t, 255


def _tiled_block(n):
    blk = _random_text(min(300, n // 16) + 1, 106, 255)[:-1]
    t = np.tile(blk, n // len(blk) + 1)[:n].copy()
    r = _rnd(107, n)
    rate = max(0.004, 8.0 / n)                    # small texts: still a handful of mutations
    mut = (r & np.uint64((1 << 20) - 1)) < np.uint64(int(rate * (1 << 20)))
    t[mut] = ((r[mut] >> np.uint64(32)) % np.uint64(255)).astype(np.uint8) + 1
    t[n - 1] = 0
    return t, 255


def _all_equal(n):
    t = np.full(n, 1, dtype=np.uint8)
    t[n - 1] = 0
    return t, 255


def _period_2(n):
    t = np.tile(np.array([1, 2], dtype=np.uint8), n // 2 + 1)[:n].copy()
    t[n - 1] = 0
    return t, 255


def _fibonacci(n):
    t = _fib_word(n)
    t[n - 1] = 0
    return t, 255


def _u16_copies(n):
    k = key_symbols(1000, "32-bit")
    t = _random_text(n, 108, 1000, np.uint16)
    return _plant_all(t, [k + 2, 3 * k] * max(1, min(16, n // 512)), 1000), 1000


# name -> (generator, index kind, intended branch); the branches of zero-runs and u16-copies are the ones the model
# gives (tests/test_sorter_cases_cpu.py holds every case to its entry here, on both engines)
GENERATORS = collections.OrderedDict([
    ("unique", (_unique, "fm", 1)),
    ("short-copies", (_short_copies, "fm", 2)),
    ("long-copies", (_long_copies, "fm", 3)),
    ("copy-of-the-tail", (_copy_of_the_tail, "fm", 3)),
    ("zero-runs", (_zero_runs, "multi", 3)),
    ("tiled-block", (_tiled_block, "fm", 4)),
    ("all-equal", (_all_equal, "fm", 5)),
    ("period-2", (_period_2, "fm", 5)),
    ("fibonacci", (_fibonacci, "fm", 5)),
    ("u16-copies", (_u16_copies, "fm", 3)),
])


def make(name, n):
    """the case `name` at length n, or None where its plants cannot keep 8 m <= n (long copies at n = 257)"""
    gen, kind, branch = GENERATORS[name]
    got = gen(n)
    if got is None:
        return None
    t, maxc = got
    assert len(t) == n and t[0] != 0 and t[n - 2] != 0 and t[n - 1] == 0
    return Case(name, n, t, maxc, kind, branch)


def small_cases():
    return [c for c in (make(name, n) for name in GENERATORS for n in SMALL_SIZES) if c is not None]


def threshold_cases():
    return [make(name, n) for name in THRESHOLD_CASES for n in THRESHOLD_SIZES]
