"""Expected results of the batched matching statistics (include/fmx.h: fmx_match_stats_batch), computed from the CPU
oracle alone -- nothing of fm_index_amd is used here.  The loop of the header for every end position i of every pattern
(slot t = off[k] - off[0] + i - 1), vectorised over the slots:

    (s, e) = (0, len);  L = 0
    for c in P[0 .. i) reversed:
        if L == max_len (max_len != 0): break
        if c > max_character: break
        s' = lf_map2(c, s); e' = lf_map2(c, e)
        if e' < s' or e' - s' < min_count: break
        s = s'; e = e'; L += 1
    out_len[t] = L;  (out_s[t], out_e[t]) = L > 0 ? (s, e) : (0, 0)

and then the seed rule when min_seed_len > 0: a slot keeps its (s, e) only if L >= min_seed_len and (i == m or
L[t + 1] <= L[t]).  One oracle lf_map2 call per step for all slots that are still alive.
tests/test_match_stats_cpu.py pins this helper against plain scans of the text."""
import numpy as np


def expect_match_stats(oi, flat, off, min_count=1, max_len=0, min_seed_len=0):
    """(lengths, s, e): numpy u64 arrays with one entry per pattern symbol, the slots of pattern k at
    off[k] - off[0] .. off[k+1] - off[0], for the patterns flat[off[k]:off[k+1]] on the oracle index `oi`"""
    mc = max(int(min_count), 1)
    flat = np.asarray(flat)
    off = np.asarray(off, dtype=np.int64)
    npat = len(off) - 1
    m = off[1:] - off[:-1]
    total = int(m.sum())
    n = len(oi)
    start = np.repeat(off[:-1], m)                             # first symbol of the slot's pattern
    end = np.arange(total, dtype=np.int64) + (off[0] if npat else 0)   # the slot's own symbol, P[i - 1]
    i = end - start + 1                                        # end position, 1 .. m
    last = i == np.repeat(m, m)
    s = np.zeros(total, dtype=np.uint64)
    e = np.full(total, n, dtype=np.uint64)
    length = np.zeros(total, dtype=np.uint64)
    alive = np.full(total, n >= mc, dtype=bool)
    cap = int(max_len) if max_len else (int(m.max()) if npat else 0)
    for t in range(cap):
        idx = np.nonzero(alive & (i > t))[0]
        if len(idx) == 0:
            break
        c = flat[end[idx] - t].astype(np.uint64)
        absent = c > np.uint64(oi.max_character)
        alive[idx[absent]] = False
        idx, c = idx[~absent], c[~absent]
        if len(idx) == 0:
            continue
        both = oi.lf_map2(np.concatenate([c, c]), np.concatenate([s[idx], e[idx]]))
        ns, ne = both[:len(idx)], both[len(idx):]
        ok = ne.astype(np.int64) - ns.astype(np.int64) >= mc
        alive[idx[~ok]] = False
        keep = idx[ok]
        s[keep], e[keep] = ns[ok], ne[ok]
        length[keep] += np.uint64(1)
    s[length == 0] = 0
    e[length == 0] = 0
    if min_seed_len:
        nxt = np.append(length[1:], np.uint64(0))
        seed = (length >= np.uint64(min_seed_len)) & (last | (nxt <= length))
        s[~seed] = 0
        e[~seed] = 0
    return length, s, e


def seeds_of(off, length, s, e):
    """[(pattern, begin, length, s, e)] of the slots with e > s, in slot order"""
    off = np.asarray(off, dtype=np.int64)
    out = []
    for k in range(len(off) - 1):
        a, b = int(off[k] - off[0]), int(off[k + 1] - off[0])
        for t in range(a, b):
            if e[t] > s[t]:
                i = t - a + 1
                out.append((k, i - int(length[t]), int(length[t]), int(s[t]), int(e[t])))
    return out
