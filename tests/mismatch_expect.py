"""Expected results of the batched mismatch search (include/fmx.h: fmx_mismatch_count_batch / fmx_mismatch_search_batch),
computed from the CPU oracle alone -- nothing of fm_index_amd is used here.  The enumeration of the header:

    enum(i, s, e, d):
        if i == 0: emit (s, e, edits); return
        p = P[i-1]
        if d < K:
            for c = 1 .. max_character ascending, c != p:
                s' = lf_map2(c, s); e' = lf_map2(c, e)
                if e' > s': enum(i-1, s', e', d+1)
        if p <= max_character:
            s' = lf_map2(p, s); e' = lf_map2(p, e)
            if e' > s': enum(i-1, s', e', d)

walked for all patterns of the batch at once: one level of the recursion is a loop over the symbols still to prepend,
and every trip makes one oracle lf_map2 call for all live nodes times all their substitution symbols, one recursive
call for the substitutions that hold a row, and one oracle call for the patterns' own symbols.  Where a node's interval
is shorter than the alphabet, only the symbols of L[s .. e) are tried: lf_map2(c, e) - lf_map2(c, s) is the number of
rows of [s, e) whose L symbol is c, on every index kind.  tests/test_mismatch_cpu.py pins this helper against a plain
scan of the text."""
import numpy as np

UNUSED = np.uint64(0xFFFFFFFFFFFFFFFF)


def _lf2(oi, c, s, e):
    both = oi.lf_map2(np.concatenate([c, c]), np.concatenate([s, e]))
    return both[:len(c)], both[len(c):]


def _candidates(oi, s, e, p):
    """(element, symbol) of every substitution to try, element-major and ascending by symbol: 1 .. max_character without
    the element's own symbol p -- and, for an interval shorter than the alphabet, without the symbols L[s .. e) lacks"""
    maxc = oi.max_character
    size = (e - s).astype(np.int64)
    small = size < maxc
    el_parts, c_parts = [], []
    big = np.nonzero(~small)[0]
    if len(big):
        el_parts.append(np.repeat(big, maxc))
        c_parts.append(np.tile(np.arange(1, maxc + 1, dtype=np.int64), len(big)))
    sm = np.nonzero(small)[0]
    if len(sm):
        el = np.repeat(sm, size[sm])
        first = np.cumsum(size[sm]) - size[sm]
        rows = s[sm].astype(np.int64)[np.repeat(np.arange(len(sm)), size[sm])] + (np.arange(len(el)) - np.repeat(first, size[sm]))
        sym = oi.get_l(rows.astype(np.uint64)).astype(np.int64)
        key = np.unique(el * (maxc + 2) + sym)
        el_parts.append(key // (maxc + 2))
        c_parts.append(key % (maxc + 2))
    el = np.concatenate(el_parts) if el_parts else np.zeros(0, dtype=np.int64)
    c = np.concatenate(c_parts) if c_parts else np.zeros(0, dtype=np.int64)
    order = np.lexsort((c, el))
    el, c = el[order], c[order]
    keep = (c >= 1) & (c != p[el])
    return el[keep], c[keep]


def _enum(oi, flat, off, pk, i, s, e, d, K):
    """the emissions of every node (pattern pk, i symbols to prepend, interval [s, e), d substitutions spent): a list
    per node of (s, e, edits) in the order of the header, edits = ((pos, sym), ...) in the order they were made"""
    maxc = oi.max_character
    out = [[] for _ in range(len(pk))]
    idx = np.arange(len(pk))
    pk, i, s, e = pk.copy(), i.copy(), s.copy(), e.copy()
    while len(idx):
        fin = i == 0
        for j in np.nonzero(fin)[0]:
            out[idx[j]].append((int(s[j]), int(e[j]), ()))
        keep = ~fin
        idx, pk, i, s, e = idx[keep], pk[keep], i[keep], s[keep], e[keep]
        if len(idx) == 0:
            break
        p = flat[off[pk] + i - 1].astype(np.int64)
        if d < K:
            rep, cc = _candidates(oi, s, e, p)
            if len(cc):
                ns, ne = _lf2(oi, cc.astype(np.uint64), s[rep], e[rep])
                ok = ne > ns
                rep, cc, ns, ne = rep[ok], cc[ok], ns[ok], ne[ok]
            if len(cc):
                sub = _enum(oi, flat, off, pk[rep], i[rep] - 1, ns, ne, d + 1, K)
                for t in range(len(cc)):
                    ed = (int(i[rep[t]]) - 1, int(cc[t]))
                    dst = out[idx[rep[t]]]
                    for fs, fe, eds in sub[t]:
                        dst.append((fs, fe, (ed,) + eds))
        inr = p <= maxc
        idx, pk, i, s, e, p = idx[inr], pk[inr], i[inr], s[inr], e[inr], p[inr]
        if len(idx):
            ns, ne = _lf2(oi, p.astype(np.uint64), s, e)
            ok = ne > ns
            idx, pk, i, s, e = idx[ok], pk[ok], i[ok] - 1, ns[ok], ne[ok]
    return out


def expect_mismatch(oi, flat, off, s0e0=None, max_mismatches=1):
    """(nint[npat], count[npat], s[total], e[total], edit[2 * total]) as numpy u64 arrays, the intervals of pattern k at
    cumsum(nint)[k - 1] ..; edit words are (pos << 32) | sym, UNUSED where a slot holds no substitution"""
    K = int(max_mismatches)
    assert 0 <= K <= 2
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
    ks = np.nonzero(e > s)[0] if n else np.zeros(0, dtype=np.int64)
    res = _enum(oi, flat, off, ks, (off[1:] - off[:-1])[ks], s[ks], e[ks], 0, K)
    nint = np.zeros(npat, dtype=np.uint64)
    count = np.zeros(npat, dtype=np.uint64)
    rs, re, red = [], [], []
    for k, em in zip(ks, res):
        nint[k] = len(em)
        count[k] = sum(b - a for a, b, _ in em)
    by_k = dict(zip(ks.tolist(), res))
    for k in range(npat):
        for a, b, eds in by_k.get(k, ()):
            rs.append(a)
            re.append(b)
            w = [(pos << 32) | sym for pos, sym in eds] + [int(UNUSED)] * (2 - len(eds))
            red.extend(w)
    return (nint, count, np.array(rs, dtype=np.uint64), np.array(re, dtype=np.uint64), np.array(red, dtype=np.uint64))


def variants(p, max_character, K):
    """every variant of pattern p with at most K substituted symbols, in the order of the header -- the enumeration
    without an index: [(variant, edits)], edits = ((pos, sym), ...).  A variant that keeps a symbol above max_character
    cannot occur and is left out."""
    p = np.asarray(p)
    out = []
    cur = p.copy()

    def rec(i, d, eds):
        if i == 0:
            out.append((cur.copy(), eds))
            return
        own = int(p[i - 1])
        if d < K:
            for c in range(1, max_character + 1):
                if c != own:
                    cur[i - 1] = c
                    rec(i - 1, d + 1, eds + ((i - 1, c),))
            cur[i - 1] = own
        if own <= max_character:
            rec(i - 1, d, eds)

    rec(len(p), 0, ())
    return out
