"""Reference for the clipped mode of mapping read pairs (include/awry_hip.h, "map read pairs, clipped"): the definition in plain
Python integers, on top of tests/clip_ref.py (the kept lists), tests/pair_ref.py (records of a text position, span intersection, the
augmented lists), tests/edit_ref.py (D and the hit rule) and tests/align_ref.py (a rescued candidate's span and runs); map_ref.py
supplies the doubled batch and the status codes.

A record is clip_ref's: (t_begin, t_end, edits, chain score, j, strand, mapq, flags, score, clip_left, clip_right), the fields of
awry_map_clip_t in their order; a candidate is clip_ref's too: (strand, j, edits, chain score, t_begin, t_end, score, clip_left,
clip_right).  proper_clip() and windows_of_clip() measure from fb and ve, the mates' 5' ends projected through their clips;
rank_pairs_clip() is the pure pair choice by score; map_pairs_clip() feeds it with the reference's kept lists and rescue hits."""
import numpy as np

from tests import align_ref as ar
from tests import clip_ref as cr
from tests import edit_ref as er
from tests import map_ref as mp
from tests import pair_ref as pr

PAIR_CLIP_MAX_UNPAIRED = 16384
MAP_PROPER_PAIR, MAP_RESCUED, MAP_MATE_UNMAPPED = pr.MAP_PROPER_PAIR, pr.MAP_RESCUED, pr.MAP_MATE_UNMAPPED
EDIT_MAX_LEN = pr.EDIT_MAX_LEN


def fb(x):
    """the 5' end of a forward record projected through its left clip (may be below 0)"""
    return x[0] - x[9]


def ve(x):
    """the 5' end of a reverse record projected through its right clip (may lie past the record)"""
    return x[1] + x[10]


def proper_clip(x, y, st, mn, mx):
    if x[5] == y[5]:
        return False
    f, v = (x, y) if x[5] == 0 else (y, x)
    return pr.rec_of(st, f[0]) == pr.rec_of(st, v[0]) and f[0] <= v[0] and f[1] <= v[1] and mn <= ve(v) - fb(f) <= mx


def insert_of(x, y):
    f, v = (x, y) if x[5] == 0 else (y, x)
    return ve(v) - fb(f)


def kept_list(cands, capped, wts, T):
    """K_m: every kept candidate in the clipped rank order, as records (the primary with its single-end MAPQ)"""
    return cr.rank_candidates(cands, capped, 2 * mp.MAP_MAX_CHAINS, wts, T)[0]


def cand_of(r):
    return (r[5], r[4], r[2], r[3], r[0], r[1], r[8], r[9], r[10])


def windows_of_clip(K0, K1, L0, L1, st, n_text, mn, mx, G, k, p=0):
    """pair_ref.windows_of over clipped records: the same slots, the windows measured from fb(x) and ve(x)"""
    K, L = (K0, K1), (L0, L1)
    out = []
    for m in (0, 1):
        Lo = L[1 - m]
        for a in range(G):
            query, first, count = 4 * p + 2 * (1 - m), 0, 0
            if a < len(K[m]) and k < Lo <= EDIT_MAX_LEN:
                x = K[m][a]
                if not any(proper_clip(x, y, st, mn, mx) for y in K[1 - m]):
                    query += 1 - x[5]
                    if x[5] == 0:
                        lo, hi = max(x[0], fb(x) + mn - Lo - k), fb(x) + mx - Lo + k
                    else:
                        lo, hi = ve(x) - mx, min(x[0], ve(x) - mn)
                    r = pr.rec_of(st, x[0])
                    r_lo, r_hi = int(st[r]) if len(st) else 0, int(st[r + 1]) if r + 1 < len(st) else n_text
                    lo, hi = max(lo, 0, r_lo), min(hi, n_text - 1, r_hi - 1)
                    if hi >= lo:
                        first, count = lo, hi - lo + 1
            out.append((query, first, count))
    return out


def rank_pairs_clip(cands0, cands1, capped0, capped1, resc, st, mn, mx, U, wts, T):
    """cands_m: mate m's candidates in any order; resc: {(t, a): the rescued record anchor a of mate 1 - t aims at mate t, or None}
    (records that exist: rescued_record() has applied T) -> ([record of mate 0 or None, of mate 1 or None], insert, [sel or None])"""
    K = (kept_list(cands0, capped0, wts, T), kept_list(cands1, capped1, wts, T))
    Kp = [pr.augmented(K[t], {a: z for (tt, a), z in resc.items() if tt == t}) for t in (0, 1)]
    if not Kp[0] and not Kp[1]:
        return [None, None], 0, [None, None]
    if not Kp[0] or not Kp[1]:
        t = 0 if Kp[0] else 1
        x, s = Kp[t][0]
        out, sel = [None, None], [None, None]
        out[t], sel[t] = x[:7] + (x[7] | MAP_MATE_UNMAPPED,) + x[8:], s
        return out, 0, sel
    order = []
    for i, (x, _) in enumerate(Kp[0]):
        for j, (y, _) in enumerate(Kp[1]):
            ok = proper_clip(x, y, st, mn, mx)
            order.append((-(x[8] + y[8] - (0 if ok else U)), not ok, i, j))
    order.sort()
    neg, improper, i, j = order[0]
    mapq = 0 if capped0 or capped1 else cr.MAPQ_MAX if len(order) < 2 else min(cr.MAPQ_MAX, 10 * (order[1][0] - neg) // (wts[0] + wts[1]))
    (x, sx), (y, sy) = Kp[0][i], Kp[1][j]
    flag = 0 if improper else MAP_PROPER_PAIR
    return ([x[:6] + (mapq, (x[7] & MAP_RESCUED) | flag) + x[8:], y[:6] + (mapq, (y[7] & MAP_RESCUED) | flag) + y[8:]],
            0 if improper else insert_of(x, y), [sx, sy])


def score_of_runs(runs, wts):
    """a #'=' - b #'X' - g (#'I' + #'D') over uint32 runs (length << 4 | BAM op)"""
    a_, b_, g_ = wts[:3]
    return sum((int(r) >> 4) * {7: a_, 8: -b_, 1: -g_, 2: -g_}[int(r) & 15] for r in runs)


def rescued_record(s, text_len, dist, strand, runs, wts, T):
    """the rescued candidate of a hit at s: the whole mate within dist edits, scored over the aligner's runs, no clips; None below T"""
    score = score_of_runs(runs, wts)
    if score < T:
        return None
    return (s, s + int(text_len), dist, 0, pr.PAIR_NO_CHAIN, strand, 0, MAP_RESCUED, score, 0, 0)


def rescue(t, query, first, count, k):
    """pair_ref.rescue without the record: (s, text_len, distance, uint32 runs) of the window's best hit, or None"""
    if not count:
        return None
    pos, d = er.hits_of(t.D(query), k, first, first + count)
    if not len(pos):
        return None
    h = min(range(len(pos)), key=lambda i: (int(d[i]), int(pos[i])))
    s, dist = int(pos[h]), int(d[h])
    text_len, runs = ar.align_triple(t, query, s, dist)
    return s, int(text_len), dist, runs


def map_pairs_clip(t, tsym, reads, chains_of, A, W, st, mn, mx, U, G, k, wts, T, memo=None):
    """t: edit_ref.Text of the text; reads interleaved -> per read (status, [record] (none or one), [uint32 runs per record]), and the
    inserts per pair"""
    per = cr.map_reads(tsym, st, reads, chains_of, A, 2 * A, W, wts, T, memo)
    dbl = mp.doubled(reads)
    out, inserts = [], []
    for p in range(len(reads) // 2):
        (s0, K0, runs0), (s1, K1, runs1) = per[2 * p], per[2 * p + 1]
        resc, rruns = {}, {}
        if G:
            wins = windows_of_clip(K0, K1, len(reads[2 * p]), len(reads[2 * p + 1]), st, t.n, mn, mx, G, k, p)
            for m in (0, 1):
                for a in range(G):
                    query, first, count = wins[m * G + a]
                    got = rescue(t, dbl[query], first, count, k)
                    z = None if got is None else rescued_record(got[0], got[1], got[2], query & 1, got[3], wts, T)
                    resc[(1 - m, a)] = z
                    rruns[(1 - m, a)] = None if z is None else got[3]
        recs, ins, sel = rank_pairs_clip([cand_of(r) for r in K0], [cand_of(r) for r in K1], s0 == mp.Q_SEED_CAP, s1 == mp.Q_SEED_CAP, resc, st, mn,
                                         mx, U, wts, T)
        for m, (status, runs) in enumerate(((s0, runs0), (s1, runs1))):
            if recs[m] is None:
                out.append((status, [], []))
            else:
                kind, at = sel[m]
                out.append((status, [recs[m]], [cr.encode(runs[at]) if kind == "c" else rruns[(m, at)]]))
        inserts.append(ins)
    return out, inserts


def as_csr(per_read, inserts):
    """-> (map_off, records MAP_CLIP_NP, cigar_off, cigar uint32, status, insert uint32)"""
    off, rows, coff, cg, st = [0], [], [0], [np.zeros(0, np.uint32)], []
    for status, recs, runs in per_read:
        st.append(status)
        rows += recs
        for r in runs:
            cg.append(np.asarray(r, np.uint32))
            coff.append(coff[-1] + len(r))
        off.append(off[-1] + len(recs))
    return (np.array(off, np.uint64), np.array(rows, cr.MAP_CLIP_NP) if rows else np.zeros(0, cr.MAP_CLIP_NP), np.array(coff, np.uint64),
            np.concatenate(cg), np.array(st, np.uint8), np.array(inserts, np.uint32))
