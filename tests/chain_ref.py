"""Reference for colinear chaining as include/awry_hip.h defines it, in plain Python integers, in two independent forms:

(a) chain_query: sort, the windowed recurrence f / p written as the header writes it, then the header's backtrack -- visit in
    descending f, walk along p, stop at a used seed;
(b) chain_query_full: a full O(N^2) table over ALL earlier seeds that records, per seed, every admissible predecessor's candidate
    and picks the result by one max over (candidate, j) tuples; the lookback is a filter on j, not a loop bound; the chains come
    from a per-seed "used" array built in visit order: each seed's chain is found by following p from it until a seed that an
    EARLIER visit has claimed.

Seeds are (q_begin, q_len, t_pos) tuples; a chain is (score, n_seeds, q_begin, q_end, t_begin, t_end, [members first to last]).
`starts` are the record starts of the index (rec(seed) = the last record that starts at or before t_pos).
Seed construction for the end-to-end tests: the records of tests/smem_ref.py and the oracle's locate lists."""
import bisect
from collections import namedtuple

import numpy as np

from tests import anchor_ref as ar

Q_SEED_CAP = 8
MAX_SEEDS, MAX_LOOKBACK = 4096, 64
Params = namedtuple("Params", "max_seeds lookback max_gap max_skew min_score")


def record_of(starts, t_pos):
    return max(0, bisect.bisect_right(starts, t_pos) - 1)


def sort_seeds(seeds):
    """ascending by (t_pos, q_begin, q_len, input index)"""
    return [seeds[i] for i in sorted(range(len(seeds)), key=lambda i: (seeds[i][2], seeds[i][0], seeds[i][1], i))]


def admissible(sj, si, rj, ri, P):
    dq, dt = si[0] - sj[0], si[2] - sj[2]
    return rj == ri and 0 < dq <= P.max_gap and 0 < dt <= P.max_gap and abs(dq - dt) <= P.max_skew


def gain(sj, si):
    dq, dt = si[0] - sj[0], si[2] - sj[2]
    return min(si[1], dq, dt) - abs(dq - dt)


def scores(s, rec, P):
    """form (a) -> (f, p, pairs evaluated) over the sorted seeds s"""
    f, p, pairs = [], [], 0
    for i, si in enumerate(s):
        fi, pi = si[1], None
        for j in range(max(0, i - P.lookback), i):  # ascending j with >=: among equals the largest j wins
            pairs += 1
            if admissible(s[j], si, rec[j], rec[i], P):
                c = f[j] + gain(s[j], si)
                if c > si[1] and c >= fi:
                    fi, pi = c, j
        f.append(fi)
        p.append(pi)
    return f, p, pairs


def backtrack(s, f, p, P):
    """form (a): the header's walk"""
    used = [False] * len(s)
    chains = []
    for e in sorted(range(len(s)), key=lambda i: (-f[i], i)):
        if used[e]:
            continue
        mem, u, base = [], e, 0
        while True:
            used[u] = True
            mem.append(u)
            if p[u] is None:
                break
            if used[p[u]]:
                base = f[p[u]]
                break
            u = p[u]
        score = f[e] - base
        if score >= P.min_score:
            chains.append(make_chain(s, score, mem[::-1]))
    return chains


def make_chain(s, score, mem):
    first = s[mem[0]]
    return (score, len(mem), first[0], max(s[m][0] + s[m][1] for m in mem), first[2], max(s[m][2] + s[m][1] for m in mem), [s[m] for m in mem])


def chain_query(seeds, starts, P):
    """form (a) -> (status, chains, (seeds chained, pairs evaluated, chains reported))"""
    if len(seeds) > P.max_seeds:
        return Q_SEED_CAP, [], (0, 0, 0)
    s = sort_seeds(seeds)
    rec = [record_of(starts, x[2]) for x in s]
    f, p, pairs = scores(s, rec, P)
    chains = backtrack(s, f, p, P)
    return 0, chains, (len(s), pairs, len(chains))


def scores_full(s, rec, P):
    """form (b): every earlier seed is looked at; the window is a condition"""
    f, p = [], []
    for i, si in enumerate(s):
        cands = [(f[j] + gain(s[j], si), j) for j in range(i) if i - j <= P.lookback and admissible(s[j], si, rec[j], rec[i], P)]
        best = max(cands) if cands else None
        if best is not None and best[0] > si[1]:
            f.append(best[0])
            p.append(best[1])
        else:
            f.append(si[1])
            p.append(None)
    return f, p


def chains_full(s, f, p, P):
    """form (b): claimed[i] = the visit rank of the chain end that claimed seed i; the chain of an end e is the path from e whose
    seeds no earlier end has claimed"""
    order = sorted(range(len(s)), key=lambda i: (-f[i], i))
    claimed = {}
    out = []
    for rank, e in enumerate(order):
        if e in claimed:
            continue
        path, u = [], e
        while u is not None and u not in claimed:
            path.append(u)
            u = p[u]
        for m in path:
            claimed[m] = rank
        score = f[e] - (f[u] if u is not None else 0)
        if score >= P.min_score:
            out.append(make_chain(s, score, path[::-1]))
    return out


def chain_query_full(seeds, starts, P):
    if len(seeds) > P.max_seeds:
        return Q_SEED_CAP, []
    s = sort_seeds(seeds)
    rec = [record_of(starts, x[2]) for x in s]
    f, p = scores_full(s, rec, P)
    return 0, chains_full(s, f, p, P)


def chain_bases(seeds, starts, P):
    """the base of every REPORTED chain of the query, in report order (base > 0: the walk stopped at a used seed)"""
    s = sort_seeds(seeds)
    rec = [record_of(starts, x[2]) for x in s]
    f, p, _ = scores(s, rec, P)
    used, bases = [False] * len(s), []
    for e in sorted(range(len(s)), key=lambda i: (-f[i], i)):
        if used[e]:
            continue
        u, base = e, 0
        while True:
            used[u] = True
            if p[u] is None:
                break
            if used[p[u]]:
                base = f[p[u]]
                break
            u = p[u]
        if f[e] - base >= P.min_score:
            bases.append(base)
    return bases


def as_csr(per_query):
    """[(status, chains)] -> (chain_off uint64[n+1], chains int64[total, 6], seed_off uint64[total+1], seeds int64[members, 3], status uint8[n])"""
    chains = [c for _, cq in per_query for c in cq]
    off = np.zeros(len(per_query) + 1, np.uint64)
    off[1:] = np.cumsum([len(cq) for _, cq in per_query], dtype=np.uint64)
    soff = np.zeros(len(chains) + 1, np.uint64)
    soff[1:] = np.cumsum([c[1] for c in chains], dtype=np.uint64)
    rows = np.array([c[:6] for c in chains], np.int64).reshape(-1, 6)
    mem = np.array([m for c in chains for m in c[6]], np.int64).reshape(-1, 3)
    return off, rows, soff, mem, np.array([st for st, _ in per_query], np.uint8)


def got_chain_rows(chains):
    """the library's CHAIN_DTYPE array -> int64[total, 6] in the column order of as_csr"""
    return np.stack([chains[f].astype(np.int64) for f in ("score", "n_seeds", "q_begin", "q_end", "t_begin", "t_end")], axis=1).reshape(-1, 6)


def got_seed_rows(seeds):
    return np.stack([seeds[f].astype(np.int64) for f in ("q_begin", "q_len", "t_pos")], axis=1).reshape(-1, 3)


def seeds_from_smems(oi, queries, per_query_smems, alphabet, max_hits):
    """per query, the seeds of its SMEM records (tests/smem_ref.py) with count <= max_hits, one per oracle locate hit, in the
    library's order: records as reported, hits in the oracle's (ascending BWT row) order"""
    hoff, g, _ = ar.locate_reference(oi, queries, per_query_smems, alphabet, max_hits)
    out, s = [], 0
    for aq in per_query_smems:
        sq = []
        for b, ln, _, _ in aq:
            sq.extend((b, ln, int(t)) for t in g[int(hoff[s]):int(hoff[s + 1])])
            s += 1
        out.append(sq)
    return out
