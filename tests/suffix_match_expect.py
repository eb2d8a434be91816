"""Expected results of the batched longest-suffix match (include/fmx.h: fmx_suffix_match_batch), computed from the CPU
oracle alone -- nothing of fm_index_amd is used here.  The loop of the header, vectorised over the batch:

    (s, e) = s0e0 ? (s0e0[2k], s0e0[2k+1]) : (0, len);  L = 0
    for c in pattern reversed:
        if c > max_character: break
        s' = lf_map2(c, s); e' = lf_map2(c, e)
        if e' - s' < min_count: break
        s = s'; e = e'; L += 1

One oracle lf_map2 call per step for all patterns that are still alive.  tests/test_suffix_match_cpu.py pins this
helper against a plain scan of the text."""
import numpy as np


def expect_suffix_match(oi, flat, off, s0e0=None, min_count=1):
    """(s, e, count, L) as numpy u64 arrays for the patterns flat[off[k]:off[k+1]] on the oracle index `oi`"""
    mc = max(int(min_count), 1)
    flat = np.asarray(flat)
    off = np.asarray(off, dtype=np.int64)
    npat = len(off) - 1
    n = len(oi)
    if s0e0 is None:
        s = np.zeros(npat, dtype=np.uint64)
        e = np.full(npat, n, dtype=np.uint64)
    else:
        se = np.asarray(s0e0, dtype=np.uint64).reshape(-1, 2)
        s, e = se[:, 0].copy(), se[:, 1].copy()
    length = np.zeros(npat, dtype=np.uint64)
    m = off[1:] - off[:-1]
    alive = np.ones(npat, dtype=bool)
    for t in range(int(m.max()) if npat else 0):
        idx = np.nonzero(alive & (m > t))[0]
        if len(idx) == 0:
            break
        c = flat[off[idx + 1] - 1 - t].astype(np.uint64)
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
    return s, e, np.where(e >= s, e - s, np.uint64(0)), length     # (a given start pair with e < s holds no row)
