"""Two independent references for substitution-tolerant search (Hamming distance <= k, include/awry_hip.h):

(a) brute_force: the definition itself -- sliding windows over the text as symbol indices, windows holding '$' excluded --
    for texts up to a few hundred kbp;
(b) variant enumeration: every string at exactly distance d from the query is counted / located with the oracle (the
    exact-match checker under oracle/), for texts of a few Mbp and short queries.

Both map bytes to symbol indices the way the exact path does (alphabet.h)."""
import itertools

import numpy as np

NT_LETTERS = b"$ACGNT"
AA_LETTERS = b"$ACDEFGHIKLMNPQRSTVWXY"


def symbol_lut(alphabet):
    """uint8[256]: byte -> symbol index (case-insensitive, U = T, '$' / '#' = 0, anything else N / X); 255 for bytes >= 0x80"""
    lut = np.zeros(256, np.uint8)
    letters = NT_LETTERS if alphabet == 0 else AA_LETTERS
    other = 4 if alphabet == 0 else 20
    for b in range(256):
        c = chr(b).upper() if b < 128 else None
        if c is None:
            lut[b] = 255
        elif c in "$#":
            lut[b] = 0
        elif alphabet == 0 and c == "U":
            lut[b] = 5
        elif c.encode() in letters[1:]:
            lut[b] = letters.index(c.encode())
        else:
            lut[b] = other
    return lut


def letters(alphabet):
    return NT_LETTERS if alphabet == 0 else AA_LETTERS


def to_symbols(x, alphabet):
    return symbol_lut(alphabet)[np.frombuffer(bytes(x), np.uint8)]


def brute_force(text, query, k, alphabet=0):
    """-> (counts uint64[k + 1] at exactly 0..k substitutions, positions int64[], distances uint8[]) sorted by position"""
    t = to_symbols(text, alphabet)
    q = to_symbols(query, alphabet)
    L, n = len(q), len(t)
    if L == 0 or L > n:
        return np.zeros(k + 1, np.uint64), np.zeros(0, np.int64), np.zeros(0, np.uint8)
    W = n - L + 1
    dist = np.zeros(W, np.int32)
    sent = np.zeros(W, bool)
    for j in range(L):
        w = t[j:j + W]
        dist += w != q[j]
        sent |= w == 0
    ok = (~sent) & (dist <= k)
    pos = np.nonzero(ok)[0]
    d = dist[pos].astype(np.uint8)
    return np.bincount(d, minlength=k + 1)[:k + 1].astype(np.uint64), pos.astype(np.int64), d


def variants(query, d, alphabet=0):
    """every string (as ASCII bytes of canonical letters) at exactly distance d from `query` over the non-sentinel symbols"""
    q = to_symbols(query, alphabet)
    lt = letters(alphabet)
    nsym = len(lt) - 1
    base = bytes(lt[s] for s in q)
    out = []
    for cols in itertools.combinations(range(len(q)), d):
        alts = [[s for s in range(1, nsym + 1) if s != q[c]] for c in cols]
        for subs in itertools.product(*alts):
            b = bytearray(base)
            for c, s in zip(cols, subs):
                b[c] = lt[s]
            out.append(bytes(b))
    return out


def variants_array(query, d, alphabet=0):
    """variants() as one uint8[nv, L] array of canonical ASCII letters, in the same order, built with numpy: sets of d columns
    in lexicographic order, and for each set the d-tuples of other symbols in lexicographic order"""
    q = to_symbols(query, alphabet).astype(np.int64)
    L = len(q)
    assert L == 0 or (int(q.min()) >= 1 and int(q.max()) < 255), "a query with '$', '#' or a byte >= 0x80 has no variants"
    lt = np.frombuffer(letters(alphabet), np.uint8)
    na = len(lt) - 2  # other symbols per column
    if d > L:
        return np.zeros((0, L), np.uint8)
    if d == 0:
        return lt[q][None, :].copy()
    cols = np.array(list(itertools.combinations(range(L), d)), np.int64).reshape(-1, d)
    subs = np.indices((na,) * d).reshape(d, -1).T                # [na ** d, d]: which of the other symbols, per column of the set
    alt = np.arange(na)[None, :] + 1 + (np.arange(na)[None, :] + 1 >= q[:, None])  # alt[j, a]: the a-th symbol other than q[j]
    out = np.empty((len(cols), len(subs), L), np.uint8)
    out[:] = lt[q]
    ci, si = np.arange(len(cols))[:, None], np.arange(len(subs))[None, :]
    for t in range(d):
        c = cols[:, t][:, None]
        out[ci, si, c] = lt[alt[c, subs[:, t][None, :]]]
    return out.reshape(-1, L)


def _query_groups(queries, k, alphabet, max_bytes):
    """cut range(len(queries)) into runs whose variant bytes (all distances 0..k) stay below max_bytes (one query may exceed it)"""
    na = len(letters(alphabet)) - 2
    lo, acc = 0, 0
    for i, q in enumerate(queries):
        L = len(q)
        nv = 1 + (L * na if k >= 1 else 0) + (L * (L - 1) // 2 * na * na if k >= 2 else 0)
        if i > lo and acc + nv * L > max_bytes:
            yield lo, i
            lo, acc = i, 0
        acc += nv * L
    if len(queries) > lo:
        yield lo, len(queries)


def oracle_search_batch(oi, queries, k, alphabet=0, threads=16, locate=False, max_bytes=256 << 20):
    """The variant-enumeration reference for a whole batch: every variant of every query counted by the oracle's
    parallel_count, in chunks of at most max_bytes of variant bytes.
    -> counts uint64[n, k + 1], leaves int64[n] (variants that occur), and with locate=True also the CSR hit lists
    (hit_off uint64[n + 1], global positions uint64[], (record, offset) uint64[, 2], distances uint8[]) in the order the
    mismatch locate promises.  That order is oracle_locate's, built without one search_range call per variant: the occurring
    variants of one query have the same length and pairwise disjoint row ranges, so ascending first row is their
    lexicographic order as symbol indices, which is byte order for canonical letters ('$' < letters, letters alphabetical);
    the oracle's parallel_locate of the variants sorted that way, concatenated, is the list."""
    n = len(queries)
    counts, leaves = np.zeros((n, k + 1), np.uint64), np.zeros(n, np.int64)
    gs, ps, ds = [], [], []
    queries = [bytes(q) for q in queries]
    for lo, hi in _query_groups(queries, k, alphabet, max_bytes):
        var, dist = [], []  # per query: its variants of every distance as one array, and the distance of each
        for q in queries[lo:hi]:
            vs = [variants_array(q, d, alphabet) for d in range(min(k, len(q)) + 1)] if len(q) else []  # (an empty query has no hit)
            var.append(np.concatenate(vs) if vs else np.zeros((0, 0), np.uint8))
            dist.append(np.concatenate([np.full(len(v), d, np.int64) for d, v in enumerate(vs)]) if vs else np.zeros(0, np.int64))
        nv = np.array([len(v) for v in var], np.int64)
        if nv.sum() == 0:
            continue
        qo = np.zeros(int(nv.sum()) + 1, np.uint64)
        qo[1:] = np.cumsum(np.repeat([v.shape[1] for v in var], nv))
        c, _ = oi.parallel_count(np.concatenate([v.reshape(-1) for v in var]), qo, threads)
        cut = np.concatenate([[0], np.cumsum(nv)])
        sel_b, sel_l, sel_d = [], [], []
        for j, (v, d) in enumerate(zip(var, dist)):
            cj = c[cut[j]:cut[j + 1]]
            counts[lo + j] = [int(cj[d == x].sum()) for x in range(k + 1)]
            present = cj > 0
            leaves[lo + j] = int(present.sum())
            if locate and present.any():
                rows = np.ascontiguousarray(v[present])
                order = np.argsort(rows.view("S%d" % v.shape[1]).ravel(), kind="stable")
                sel_b.append(rows[order].reshape(-1))
                sel_l.append(np.full(len(order), v.shape[1], np.int64))
                sel_d.append(d[present][order])
        if sel_b:
            sel_l, sel_d = np.concatenate(sel_l), np.concatenate(sel_d)
            so = np.zeros(len(sel_l) + 1, np.uint64)
            so[1:] = np.cumsum(sel_l)
            off, g, p, _ = oi.parallel_locate(np.concatenate(sel_b), so, threads)
            gs.append(g)
            ps.append(p)
            ds.append(np.repeat(sel_d, np.diff(off.astype(np.int64))).astype(np.uint8))
    if not locate:
        return counts, leaves
    hit_off = np.zeros(n + 1, np.uint64)
    hit_off[1:] = np.cumsum(counts.sum(axis=1))
    g = np.concatenate(gs).astype(np.uint64) if gs else np.zeros(0, np.uint64)
    assert len(g) == int(hit_off[-1])  # every located variant was counted at the same width, query by query in order
    return (counts, leaves, hit_off, g, np.concatenate(ps) if ps else np.zeros((0, 2), np.uint64),
            np.concatenate(ds) if ds else np.zeros(0, np.uint8))


def oracle_counts_batch(oi, queries, k, alphabet=0, threads=16, max_bytes=256 << 20):
    """-> (counts uint64[n, k + 1], leaves int64[n]): oracle_counts for a batch, see oracle_search_batch"""
    return oracle_search_batch(oi, queries, k, alphabet, threads, False, max_bytes)


def oracle_counts(oi, query, k, alphabet=0):
    """counts uint64[k + 1] from the oracle's exact counts of all variants"""
    out = np.zeros(k + 1, np.uint64)
    for d in range(min(k, len(query)) + 1):
        vs = variants(query, d, alphabet)
        if not vs:
            continue
        qb = np.frombuffer(b"".join(vs), np.uint8)
        qo = np.arange(len(vs) + 1, dtype=np.uint64) * np.uint64(len(query))
        c, _ = oi.parallel_count(qb, qo)
        out[d] = int(c.sum())
    return out


def oracle_locate(oi, query, k, alphabet=0):
    """-> (global positions, (record, offset) pairs, distances) in the order the mismatch locate promises: the oracle's
    per-variant locate lists concatenated in ascending range-start order"""
    found = []
    for d in range(min(k, len(query)) + 1):
        vs = variants(query, d, alphabet)
        if not vs:
            continue
        qb = np.frombuffer(b"".join(vs), np.uint8)
        qo = np.arange(len(vs) + 1, dtype=np.uint64) * np.uint64(len(query))
        c, _ = oi.parallel_count(qb, qo)
        for v, cnt in zip(vs, c):
            if cnt:
                sp, _ = oi.search_range(v)
                g, p = oi.locate_string(v)
                found.append((sp, g, p, d))
    found.sort(key=lambda x: x[0])
    gp = np.concatenate([f[1] for f in found]) if found else np.zeros(0, np.uint64)
    pos = np.array([pp for f in found for pp in f[2]], np.uint64).reshape(-1, 2)
    dist = np.concatenate([np.full(len(f[1]), f[3], np.uint8) for f in found]) if found else np.zeros(0, np.uint8)
    return gp.astype(np.uint64), pos, dist


def assert_hits_are_the_definition(text, alphabet, q2d, k, counts, off, gpos, dist):
    """A locate result of the equal-length queries q2d checked against the text itself, given the reference's counts
    (uint64[n, >= k + 1]): per query as many hits as counted, per distance; the hits of one query distinct; every hit's window
    free of '$' and at exactly the reported distance (<= k) from the query.  Together: the hit set is the definition's."""
    lut = symbol_lut(alphabet)
    n, L = q2d.shape
    lens = np.diff(off.astype(np.int64))
    assert len(lens) == n and np.array_equal(lens, counts[:, :k + 1].sum(axis=1).astype(np.int64))
    assert len(gpos) == len(dist) == int(off[-1])
    qi = np.repeat(np.arange(n), lens)
    g = gpos.astype(np.int64)
    order = np.lexsort((g, qi))
    gs, qs = g[order], qi[order]
    assert not ((gs[1:] == gs[:-1]) & (qs[1:] == qs[:-1])).any(), "a position reported twice for one query"
    assert len(g) == 0 or (int(g.min()) >= 0 and int(g.max()) + L <= len(text))
    qsym = lut[q2d]
    for a in range(0, len(g), 1 << 21):
        e = min(len(g), a + (1 << 21))
        win = lut[text[g[a:e, None] + np.arange(L)[None, :]]]
        assert (win != 0).all(), "a hit's window holds '$'"
        dd = (win != qsym[qi[a:e]]).sum(axis=1)
        assert np.array_equal(dd, dist[a:e].astype(np.int64)) and (dd <= k).all()
    per = np.zeros((n, k + 1), np.int64)
    np.add.at(per, (qi, dist.astype(np.int64)), 1)
    assert np.array_equal(per, counts[:, :k + 1].astype(np.int64))


def budgeted_rows(tot, light, budget, seed):
    """rows of a sample to locate under a host-memory budget of `budget` hits: every query with at most `light` hits, then
    heavier ones in a seeded random order while the budget lasts -> (sorted rows, number of heavier ones)"""
    tot = np.asarray(tot, np.int64)
    rows = np.flatnonzero(tot <= light)
    left, heavy = budget - int(tot[rows].sum()), []
    assert left >= 0
    for i in np.random.default_rng(seed).permutation(np.flatnonzero(tot > light)).tolist():
        if int(tot[i]) <= left:
            heavy.append(i)
            left -= int(tot[i])
    return np.sort(np.concatenate([rows, np.array(heavy, dtype=np.int64)])), len(heavy)
