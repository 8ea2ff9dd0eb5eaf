"""Reference for split reads (include/awry_hip.h, "split reads: supplementary alignments by query overlap"): the walk over the ranked
clipped candidates of a read by query interval, in plain Python integers, stated twice, on top of tests/clip_ref.py.

walk() is the definition as the header states it: one pass over the ranked list, the segments so far in a list, the first overlapping
one found by scanning it.  walk_matrix() differs in method: it first builds, over all candidates that pass the threshold, the full
matrices of query overlap (in exact fractions) and of same-strand text intersection, gives every candidate the SET of all segments it
overlaps, and derives the parent (the set's minimum), every segment's sub (the maximum score among its secondaries), the report order
and MAPQ from those sets afterwards.
A candidate is clip_ref's tuple (strand, j, edits, chain score, t_begin, t_end, score, clip_left, clip_right); a record is the fields of
awry_map_split_t in their order."""
from fractions import Fraction

import numpy as np

from tests import chain_align_ref as ca
from tests import clip_ref as cl
from tests import map_ref as mp

MAPQ_MAX = 60
MAP_SUPPLEMENTARY = 16
MAX_SEGMENTS = 4
MAX_READ = 0xFFFF  # a longer read counts as this long: the interval is two 16-bit fields

MAP_SPLIT_NP = np.dtype(cl.MAP_CLIP_NP.descr + [("q_begin", "<u2"), ("q_end", "<u2"), ("parent", "<u2"), ("reserved", "<u2")])


def rank_key(c):
    return (-c[6], c[2], c[0], c[4], c[1])


def interval(c, L):
    """[q_begin, q_end) of candidate c in the read's own orientation; both clips saturate at L"""
    L = min(L, MAX_READ)
    lo, hi = (c[7], c[8]) if c[0] == 0 else (c[8], c[7])
    qb = min(lo, L)
    return qb, max(qb, L - min(hi, L))


def overlaps(b1, e1, b2, e2, O):
    ov = min(e1, e2) - max(b1, b2)
    return ov > 0 and 100 * ov >= O * min(e1 - b1, e2 - b2)


def text_intersects(c, k):
    return k[0] == c[0] and max(k[4], c[4]) < min(k[5], c[5])


def _records(segs, secs, subs, capped, R2, wts):
    """segs: [(c, qb, qe)] in acceptance order, secs: [(c, qb, qe, parent)] in rank order, subs[x]: the score or None"""
    out = []
    for x, (c, qb, qe) in enumerate(segs):
        mapq = 0 if capped else MAPQ_MAX if subs[x] is None else min(MAPQ_MAX, 10 * (c[6] - subs[x]) // (wts[0] + wts[1]))
        out.append((c[4], c[5], c[2], c[3], c[1], c[0], mapq, MAP_SUPPLEMENTARY if x else 0, c[6], c[7], c[8], qb, qe, x, 0))
    for c, qb, qe, x in secs[:R2]:
        out.append((c[4], c[5], c[2], c[3], c[1], c[0], 0, mp.MAP_SECONDARY, c[6], c[7], c[8], qb, qe, x, 0))
    return out


def walk(cands, capped, L, P, R2, O, wts, T):
    """-> (records, stats); stats counts what the walk did: segments, secondaries, and the candidates dropped for an empty interval,
    for redundancy and at the segment cap"""
    order = sorted((c for c in cands if c[6] >= T), key=rank_key)
    kept, segs, subs, secs = [], [], [], []
    stats = dict(empty=0, redundant=0, capped=0)
    for c in order:
        qb, qe = interval(c, L)
        if qe == qb:
            stats["empty"] += 1
            continue
        if any(text_intersects(c, k) for k in kept):
            stats["redundant"] += 1
            continue
        x = next((x for x, (_, gb, ge) in enumerate(segs) if overlaps(qb, qe, gb, ge, O)), None)
        if x is None:
            if len(segs) >= P:
                stats["capped"] += 1
                continue
            segs.append((c, qb, qe))
            subs.append(None)
        else:
            if subs[x] is None:
                subs[x] = c[6]
            secs.append((c, qb, qe, x))
        kept.append(c)
    stats.update(segments=len(segs), secondaries=len(secs))
    return _records(segs, secs, subs, capped, R2, wts), stats


def walk_matrix(cands, capped, L, P, R2, O, wts, T):
    """the second form -> (records, per kept secondary the set of all segments it overlaps)"""
    pool = [c for c in cands if c[6] >= T]
    m = len(pool)
    iv = [interval(c, L) for c in pool]
    span = [e - b for b, e in iv]
    # the full matrices, over all pairs: overlap as an exact fraction of the shorter interval, text intersection per strand
    frac = [[Fraction(max(0, min(iv[a][1], iv[b][1]) - max(iv[a][0], iv[b][0])), min(span[a], span[b])) if span[a] and span[b] else Fraction(0)
             for b in range(m)] for a in range(m)]
    over = [[frac[a][b] > 0 and frac[a][b] >= Fraction(O, 100) for b in range(m)] for a in range(m)]
    hit = [[pool[a][0] == pool[b][0] and not (pool[a][5] <= pool[b][4] or pool[b][5] <= pool[a][4]) and pool[a][5] > pool[a][4] and pool[b][5] > pool[b][4]
            for b in range(m)] for a in range(m)]
    rank = sorted(range(m), key=lambda a: rank_key(pool[a]))
    kept, seg_ids, sets = [], [], {}
    for a in rank:
        if not span[a] or any(hit[a][k] for k in kept):
            continue
        mine = {x for x, g in enumerate(seg_ids) if over[a][g]}
        if not mine:
            if len(seg_ids) == P:
                continue
            seg_ids.append(a)
        else:
            sets[a] = mine
        kept.append(a)
    secs_ids = [a for a in rank if a in sets]  # rank order
    parent = {a: min(sets[a]) for a in secs_ids}
    subs = [max([pool[a][6] for a in secs_ids if parent[a] == x], default=None) for x in range(len(seg_ids))]
    segs = [(pool[g],) + iv[g] for g in seg_ids]
    secs = [(pool[a],) + iv[a] + (parent[a],) for a in secs_ids]
    return _records(segs, secs, subs, capped, R2, wts), [sets[a] for a in secs_ids]


def candidates_of(aln_off, chains, alns, i, A):
    cands = []
    for s in (0, 1):
        lo, hi = int(aln_off[2 * i + s]), int(aln_off[2 * i + s + 1])
        for j, c in enumerate(range(lo, min(hi, lo + A))):
            if int(alns[c]["status"]) == ca.ALN_OK:
                cands.append((s, j, int(alns[c]["edits"]), int(chains[c]["score"]), int(alns[c]["t_begin"]), int(alns[c]["t_end"]), int(alns[c]["score"]),
                              int(alns[c]["clip_left"]), int(alns[c]["clip_right"])))
    return cands


def rank_alignments(aln_off, chains, alns, chain_status, lengths, n, A, P, R2, O, wts, T, stats=None):
    """the pure walk over the arrays awry_align_chains_clip_batch returns for the doubled batch of n reads of the given lengths
    -> (map_off uint64[n+1], records MAP_SPLIT_NP, per record the index of its alignment, status uint8[n]); stats (a list) receives the
    walk's counts per read"""
    off, rows, sel, st = [0], [], [], []
    for i in range(n):
        capped = mp.Q_SEED_CAP in (int(chain_status[2 * i]), int(chain_status[2 * i + 1]))
        recs, s = walk(candidates_of(aln_off, chains, alns, i, A), capped, int(lengths[i]), P, R2, O, wts, T)
        if stats is not None:
            stats.append(s)
        rows += recs
        sel += [int(aln_off[2 * i + r[5]]) + r[4] for r in recs]
        off.append(off[-1] + len(recs))
        st.append(mp.Q_SEED_CAP if capped else mp.Q_OK)
    return np.array(off, np.uint64), np.array(rows, MAP_SPLIT_NP) if rows else np.zeros(0, MAP_SPLIT_NP), sel, np.array(st, np.uint8)


def map_reads(tsym, seq_starts, reads, chains_of, A, P, R2, O, W, wts, T, memo=None):
    """chains_of(queries) -> tests/chain_ref.py's [(status, chains)] per query.  -> per read (status, [record], [runs per record])"""
    qs = mp.doubled(reads)
    al = cl.align_queries(tsym, seq_starts, qs, chains_of(qs), A, W, wts, memo)
    out = []
    for i in range(len(reads)):
        cands, runs = [], {}
        for s in (0, 1):
            for j, (c, g) in enumerate(al[2 * i + s][1]):
                if g[0] == ca.ALN_OK:
                    cands.append((s, j, g[3], c[0], g[1], g[2], g[6], g[7], g[8]))
                    runs[(s, j)] = g[4]
        capped = mp.Q_SEED_CAP in (al[2 * i][0], al[2 * i + 1][0])
        recs, _ = walk(cands, capped, len(reads[i]), P, R2, O, wts, T)
        out.append((mp.Q_SEED_CAP if capped else mp.Q_OK, recs, [runs[(r[5], r[4])] for r in recs]))
    return out


def as_csr(per_read):
    """[(status, records, runs)] -> (map_off, records MAP_SPLIT_NP, cigar_off, cigar uint32, status)"""
    off, rows, coff, cg, st = [0], [], [0], [np.zeros(0, np.uint32)], []
    for status, recs, runs in per_read:
        st.append(status)
        rows += recs
        for r in runs:
            cg.append(cl.encode(r))
            coff.append(coff[-1] + len(r))
        off.append(off[-1] + len(recs))
    return (np.array(off, np.uint64), np.array(rows, MAP_SPLIT_NP) if rows else np.zeros(0, MAP_SPLIT_NP), np.array(coff, np.uint64), np.concatenate(cg),
            np.array(st, np.uint8))
