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
