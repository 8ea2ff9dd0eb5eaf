"""Reference for mapping read pairs (include/awry_hip.h, "map read pairs"): the definition in plain Python integers, on top of
tests/map_ref.py (the kept lists), tests/edit_ref.py (D and the hit rule over the whole text) and tests/align_ref.py (a rescued
candidate's span and runs).

A record is map_ref's: (t_begin, t_end, edits, chain score, j, strand, mapq, flags), the fields of awry_map_t in their order; a
candidate is map_ref's too: (strand, j, edits, score, t_begin, t_end).  windows_of() is the anchor rule and the window arithmetic
of one pair; rank_pairs() is the pure pair choice -- candidate lists and rescued candidates in, records out; map_pairs() feeds it
with the reference's kept lists and rescue hits."""
import bisect

import numpy as np

from tests import align_ref as ar
from tests import chain_align_ref as ca
from tests import edit_ref as er
from tests import map_ref as mp

PAIR_MAX_INSERT, PAIR_MAX_ANCHORS, PAIR_NO_CHAIN = 1 << 20, 4, 0xFFFFFFFF
MAP_PROPER_PAIR, MAP_RESCUED, MAP_MATE_UNMAPPED = 2, 4, 8
EDIT_MAX_LEN, MAX_EDITS = 256, 8
SEL_RESCUED = 0x80000000


def rec_of(st, t):
    """the record awry_get_seq_location(t) returns: the largest i with st[i] <= t"""
    return max(bisect.bisect_right([int(x) for x in st], t) - 1, 0)


def proper(x, y, st, mn, mx):
    if x[5] == y[5]:
        return False
    f, v = (x, y) if x[5] == 0 else (y, x)
    return rec_of(st, f[0]) == rec_of(st, v[0]) and f[0] <= v[0] and f[1] <= v[1] and mn <= v[1] - f[0] <= mx


def insert_of(x, y):
    f, v = (x, y) if x[5] == 0 else (y, x)
    return v[1] - f[0]


def intersects(a, b):
    return a[5] == b[5] and max(a[0], b[0]) < min(a[1], b[1])


def kept_list(cands, capped):
    """K_m: every kept candidate in rank order, as records (the primary with its single-end MAPQ)"""
    return mp.rank_candidates(cands, capped, 2 * mp.MAP_MAX_CHAINS)[0]


def cand_of(r):
    return (r[5], r[4], r[2], r[3], r[0], r[1])


def windows_of(K0, K1, L0, L1, st, n_text, mn, mx, G, k, p=0):
    """the 2 G window slots of pair p, slot (m, a) at index m G + a -> [(doubled-batch query, first, count)]; count 0 where
    candidate a of mate m is no anchor or its window is empty"""
    K, L = (K0, K1), (L0, L1)
    out = []
    for m in (0, 1):
        Lo = L[1 - m]
        for a in range(G):
            query, first, count = 4 * p + 2 * (1 - m), 0, 0
            if a < len(K[m]) and k < Lo <= EDIT_MAX_LEN:
                x = K[m][a]
                if not any(proper(x, y, st, mn, mx) for y in K[1 - m]):
                    query += 1 - x[5]
                    if x[5] == 0:
                        lo, hi = x[0] + max(0, mn - Lo - k), x[0] + mx - Lo + k
                    else:
                        lo, hi = x[1] - mx, min(x[0], x[1] - mn)
                    r = rec_of(st, x[0])
                    r_lo, r_hi = int(st[r]) if len(st) else 0, int(st[r + 1]) if r + 1 < len(st) else n_text
                    lo, hi = max(lo, 0, r_lo), min(hi, n_text - 1, r_hi - 1)
                    if hi >= lo:
                        first, count = lo, hi - lo + 1
            out.append((query, first, count))
    return out


def augmented(K, resc_t):
    """K'_t: [(record, sel)] -- sel = ("c", index in K_t) or ("r", anchor index a) -- resc_t: {a: rescued record aimed at mate t}"""
    lst = [(r, ("c", i)) for i, r in enumerate(K)]
    for a in sorted(resc_t):
        z = resc_t[a]
        if z is not None and not any(intersects(z, o) for o, _ in lst):
            lst.append((z, ("r", a)))
    return lst


def rank_pairs(cands0, cands1, capped0, capped1, resc, st, mn, mx, U):
    """cands_m: mate m's candidates in any order (the rank is a total order); resc: {(t, a): the rescued record anchor a of mate 1 - t
    aims at mate t, or None} -> ([record of mate 0 or None, record of mate 1 or None], insert, [sel of each record or None])"""
    K = (kept_list(cands0, capped0), kept_list(cands1, capped1))
    Kp = [augmented(K[t], {a: z for (tt, a), z in resc.items() if tt == t}) for t in (0, 1)]
    if not Kp[0] and not Kp[1]:
        return [None, None], 0, [None, None]
    if not Kp[0] or not Kp[1]:
        t = 0 if Kp[0] else 1
        x, s = Kp[t][0]
        out, sel = [None, None], [None, None]
        out[t], sel[t] = x[:7] + (x[7] | MAP_MATE_UNMAPPED,), s
        return out, 0, sel
    order = sorted((x[2] + y[2] + (0 if proper(x, y, st, mn, mx) else U), not proper(x, y, st, mn, mx), i, j)
                   for i, (x, _) in enumerate(Kp[0]) for j, (y, _) in enumerate(Kp[1]))
    cost, improper, i, j = order[0]
    mapq = 0 if capped0 or capped1 else mp.MAPQ_MAX if len(order) < 2 else min(mp.MAPQ_MAX, 10 * (order[1][0] - cost))
    (x, sx), (y, sy) = Kp[0][i], Kp[1][j]
    flag = 0 if improper else MAP_PROPER_PAIR
    return ([x[:6] + (mapq, (x[7] & MAP_RESCUED) | flag), y[:6] + (mapq, (y[7] & MAP_RESCUED) | flag)], 0 if improper else insert_of(x, y), [sx, sy])


def rescue(t, query, first, count, k):
    """the rescue hit of a window over an edit_ref.Text -> (rescued record without its strand, uint32 runs) or None"""
    if not count:
        return None
    pos, d = er.hits_of(t.D(query), k, first, first + count)
    if not len(pos):
        return None
    h = min(range(len(pos)), key=lambda i: (int(d[i]), int(pos[i])))
    s, dist = int(pos[h]), int(d[h])
    text_len, runs = ar.align_triple(t, query, s, dist)
    return (s, s + int(text_len), dist, 0, PAIR_NO_CHAIN), runs


def map_pairs(t, tsym, reads, chains_of, A, W, st, mn, mx, U, G, k, memo=None):
    """t: edit_ref.Text of the text; reads interleaved -> per read (status, [record] (none or one), [uint32 runs per record]), and the
    inserts per pair"""
    per = mp.map_reads(tsym, reads, chains_of, A, 2 * A, W, memo)
    dbl = mp.doubled(reads)
    out, inserts = [], []
    for p in range(len(reads) // 2):
        (s0, K0, runs0), (s1, K1, runs1) = per[2 * p], per[2 * p + 1]
        resc, rruns = {}, {}
        if G:
            wins = windows_of(K0, K1, len(reads[2 * p]), len(reads[2 * p + 1]), st, t.n, mn, mx, G, k, p)
            for m in (0, 1):
                for a in range(G):
                    query, first, count = wins[m * G + a]
                    got = rescue(t, dbl[query], first, count, k)
                    resc[(1 - m, a)] = None if got is None else got[0] + (query & 1, 0, MAP_RESCUED)
                    rruns[(1 - m, a)] = None if got is None else got[1]
        recs, ins, sel = rank_pairs([cand_of(r) for r in K0], [cand_of(r) for r in K1], s0 == mp.Q_SEED_CAP, s1 == mp.Q_SEED_CAP, resc, st, mn, mx, U)
        for m, (status, runs) in enumerate(((s0, runs0), (s1, runs1))):
            if recs[m] is None:
                out.append((status, [], []))
            else:
                kind, at = sel[m]
                out.append((status, [recs[m]], [ca.encode(runs[at]) if kind == "c" else rruns[(m, at)]]))
        inserts.append(ins)
    return out, inserts


def as_csr(per_read, inserts):
    """-> (map_off, records MAP_NP, cigar_off, cigar uint32, status, insert uint32)"""
    off, rows, coff, cg, st = [0], [], [0], [np.zeros(0, np.uint32)], []
    for status, recs, runs in per_read:
        st.append(status)
        rows += recs
        for r in runs:
            cg.append(np.asarray(r, np.uint32))
            coff.append(coff[-1] + len(r))
        off.append(off[-1] + len(recs))
    return (np.array(off, np.uint64), np.array(rows, mp.MAP_NP) if rows else np.zeros(0, mp.MAP_NP), np.array(coff, np.uint64), np.concatenate(cg),
            np.array(st, np.uint8), np.array(inserts, np.uint32))
