"""Reference for the clipped mode of chain alignment and mapping (include/awry_hip.h, "soft-clip read ends"): the definition in
plain Python integers, stated twice, on top of tests/chain_align_ref.py and tests/map_ref.py.

Pieces and gaps are chain_align_ref's.  The two end extensions are scored and local: H[i][j] = max(H[i-1][j-1] + (a | -b), H[i-1][j] -
g, H[i][j-1] - g) inside the band -W <= j - i <= W and the columns 0 .. J = min(a + W, avail), avail cut at the record of the first
piece's text start.  The extension ends at (a, j_e) if H_e + E >= H*, else at the best cell (ties: the largest i, then the smallest j),
and the query letters beyond are soft-clipped.

extension(..., full=False) keeps one row of 2 W + 1 cells and a direction per cell, runs only the rows up to J + W and tracks the best
cell as it goes, as the kernel does; full=True fills the whole (a + 1) x (J + 1) table with the band as a condition on cells, finds the
best cell by a scan and traces back by comparing values.  rank_candidates() is the pure ranking function of the map level.
A weight tuple is wts = (a, b, g, E).  Runs are (length, op letter) with the letters of chain_align_ref plus 'S' (BAM op 4)."""
import numpy as np

from tests import chain_align_ref as ca
from tests import map_ref as mp
from tests import mismatch_ref as mr

NEG = -(1 << 28)
OP_CODE = dict(ca.OP_CODE, S=4)
MAPQ_MAX = 60
MAX_MATCH, MAX_PENALTY, MAX_END_BONUS = 16, 64, 1024

ALN_CLIP_NP = np.dtype([("t_begin", "<u8"), ("t_end", "<u8"), ("edits", "<u4"), ("status", "<u4"), ("score", "<i4"), ("clip_left", "<u2"),
                        ("clip_right", "<u2")])
MAP_CLIP_NP = np.dtype([("t_begin", "<u8"), ("t_end", "<u8"), ("edits", "<u4"), ("chain_score", "<u4"), ("chain_index", "<u4"), ("strand", "u1"),
                        ("mapq", "u1"), ("flags", "<u2"), ("score", "<i4"), ("clip_left", "<u2"), ("clip_right", "<u2")])


def same(x, y):
    """letters compare as in the end-to-end pass: equal symbol indices, and a sentinel (0) matches nothing"""
    return x == y and x > 0


def _ext_banded(x, y, J, W, wts):
    a_, b_, g_, E = wts
    a, lo, NB = len(x), -W, 2 * W + 1
    h = [-(b + lo) * g_ if 0 <= b + lo <= J else NEG for b in range(NB)]  # row 0
    dirs = [None]
    best = (0, 0, 0)  # (H, i, j): the cell (0, 0)
    rows = min(a, J + W)
    for i in range(1, rows + 1):
        new, d, left = [NEG] * NB, [3] * NB, NEG
        for b in range(NB):
            j = i + b + lo
            if j < 0 or j > J:
                left = NEG
                continue
            if j == 0:
                v, dr = -i * g_, 2  # column 0: only 'I' leads back
            else:
                eq = same(x[i - 1], y[j - 1])
                dg = h[b] + (a_ if eq else -b_) if h[b] > NEG else NEG
                up = h[b + 1] - g_ if b + 1 < NB and h[b + 1] > NEG else NEG
                lf = left - g_ if left > NEG else NEG
                v = max(dg, up, lf)
                assert v > NEG
                dr = (0 if eq else 1) if dg == v else 2 if up == v else 3
            new[b], d[b], left = v, dr, v
            if v > best[0] or (v == best[0] and i > best[1]):
                best = (v, i, j)
        h = new
        dirs.append(d)
    he = None
    if rows == a:  # row a has a cell
        he = max(h)
        je = a + h.index(he) + lo  # the first maximum: the smallest end column
        assert he > NEG
    if he is not None and he + E >= best[0]:
        end = (he, a, je)
    else:
        end = best
    score, i, j = end
    ie, jstar, ops = i, j, []
    while i or j:
        dr = dirs[i][j - i - lo] if i else 3  # row 0: only 'D' leads back
        ops.append("=XID"[dr])
        if dr <= 1:
            i, j = i - 1, j - 1
        elif dr == 2:
            i -= 1
        else:
            j -= 1
        assert j >= 0 and lo <= j - i <= W
    return ie, jstar, score, ops, (best[0], he)


def table(x, y, J, W, wts):
    """H[i][j], 0 <= i <= len(x), 0 <= j <= J; NEG outside the band"""
    a_, b_, g_, _ = wts
    a = len(x)
    H = [[NEG] * (J + 1) for _ in range(a + 1)]
    for i in range(a + 1):
        for j in range(J + 1):
            if not -W <= j - i <= W:
                continue
            if i == 0 and j == 0:
                H[i][j] = 0
                continue
            v = NEG
            if i and j and H[i - 1][j - 1] > NEG:
                v = max(v, H[i - 1][j - 1] + (a_ if same(x[i - 1], y[j - 1]) else -b_))
            if i and H[i - 1][j] > NEG:
                v = max(v, H[i - 1][j] - g_)
            if j and H[i][j - 1] > NEG:
                v = max(v, H[i][j - 1] - g_)
            H[i][j] = v
    return H


def _ext_full(x, y, J, W, wts):
    a_, b_, g_, E = wts
    a = len(x)
    H = table(x, y, J, W, wts)
    hstar = max(v for row in H for v in row)
    istar = max(i for i in range(a + 1) if hstar in H[i])
    jstar = H[istar].index(hstar)
    he = max(H[a])
    if he > NEG and he + E >= hstar:
        i, j, score = a, H[a].index(he), he
    else:
        i, j, score = istar, jstar, hstar
    ie, je, ops = i, j, []
    while i or j:
        if i and j and H[i - 1][j - 1] > NEG and H[i - 1][j - 1] + (a_ if same(x[i - 1], y[j - 1]) else -b_) == H[i][j]:
            ops.append("=" if same(x[i - 1], y[j - 1]) else "X")
            i, j = i - 1, j - 1
        elif i and H[i - 1][j] > NEG and H[i - 1][j] - g_ == H[i][j]:
            ops.append("I")
            i -= 1
        else:
            assert j and H[i][j - 1] > NEG and H[i][j - 1] - g_ == H[i][j]
            ops.append("D")
            j -= 1
    return ie, je, score, ops, (hstar, he if he > NEG else None)


def extension(x, y, J, W, wts, full=False):
    """x (a symbols, outward from the piece) against the prefixes of y[0..J) -> (i_end, j_end, score, operations from the end cell
    back to (0, 0), (H*, H_e or None)); a - i_end letters are clipped"""
    return (_ext_full if full else _ext_banded)(list(x), list(y), J, W, wts)


def record_of(seq_starts, n, t):
    """the record of text position t as [lo, hi): the largest r with seq_starts[r] <= t; the last record ends at n"""
    r = max(k for k in range(len(seq_starts)) if int(seq_starts[k]) <= t) if len(seq_starts) else 0
    lo = int(seq_starts[r]) if len(seq_starts) else 0
    return lo, int(seq_starts[r + 1]) if r + 1 < len(seq_starts) else n


def align_chain(tsym, seq_starts, qsym, members, W, wts, full=False):
    """-> (status, t_begin, t_end, edits, [(length, op letter)], table cells, score, clip_left, clip_right) of one chain"""
    a_, b_, g_, _ = wts
    n, L = len(tsym), len(qsym)
    status, pcs = ca.pieces_of(members, L, n)
    if status:
        return status, 0, 0, 0, [], 0, 0, 0, 0
    tb, te = pcs[0][2], pcs[-1][2] + pcs[-1][1]
    qb0, qe_last = pcs[0][0], pcs[-1][0] + pcs[-1][1]
    skews = [(t1 - (t0 + l0)) - (q1 - (q0 + l0)) for (q0, l0, t0), (q1, _, t1) in zip(pcs, pcs[1:])]
    if skews and max(abs(m) for m in skews) > ca.MAX_SKEW:  # from gaps only
        return ca.ALN_SKEW, tb, te, 0, [], 0, 0, 0, 0
    rlo, rhi = record_of(seq_starts, n, min(tb, n))
    ops, cells, clip_left, clip_right = [], 0, 0, 0
    t_begin, t_end = tb, te
    if qb0:
        a, avail = qb0, tb - rlo
        J = min(a + W, avail)
        x = [qsym[qb0 - 1 - i] for i in range(a)]
        y = [tsym[tb - 1 - j] for j in range(J)]
        ie, je, _, sops, _ = extension(x, y, J, W, wts, full)
        clip_left = a - ie
        ops += ["S"] * clip_left + sops  # reversed strings: the traceback's order is the query's
        cells += ca.cells_of(a, J, 0, W)
        t_begin = tb - je
    for k, (qb, ln, tp) in enumerate(pcs):
        if k:
            q0, t0 = pcs[k - 1][0] + pcs[k - 1][1], pcs[k - 1][2] + pcs[k - 1][1]
            a, b = qb - q0, tp - t0
            _, _, sops = ca.segment(qsym[q0:qb], tsym[t0:tp], b, b - a, W, b, full)
            ops += sops[::-1]
            cells += ca.cells_of(a, b, b - a, W)
        ops += ["=" if same(qsym[qb + i], tsym[tp + i]) else "X" for i in range(ln)]
    if qe_last < L:
        a, avail = L - qe_last, max(0, rhi - te)
        J = min(a + W, avail)
        ie, je, _, sops, _ = extension(qsym[qe_last:], tsym[te:te + J], J, W, wts, full)
        clip_right = a - ie
        ops += sops[::-1] + ["S"] * clip_right
        cells += ca.cells_of(a, J, 0, W)
        t_end = te + je
    edits = sum(c in "XID" for c in ops)
    score = sum({"=": a_, "X": -b_, "I": -g_, "D": -g_, "S": 0}[c] for c in ops)
    return ca.ALN_OK, t_begin, t_end, edits, rle(ops, clip_right), cells, score, clip_left, clip_right


def rle(ops, clip_right=0):
    """run lengths over the script; an 'S' run never merges with another run (the right one is the script's last clip_right letters)"""
    runs = []
    for k, c in enumerate(ops):
        if runs and runs[-1][1] == c and not (c == "S" and k == len(ops) - clip_right):
            runs[-1][0] += 1
        else:
            runs.append([1, c])
    return [(ln, c) for ln, c in runs]


def encode(runs):
    return np.array([ln << 4 | OP_CODE[c] for ln, c in runs], np.uint32)


def cigar_text(runs):
    return "".join("%d%s" % (ln, c) for ln, c in runs)


def replay(qsym, tsym, t_begin, runs, wts):
    """walk the script over q and T[t_begin ..) -> (query letters consumed with the clips, text end, edits, score, clip_left,
    clip_right); asserts '=' / 'X' letter by letter and that 'S' runs stand only first and last.  A first 'S' run counts as the left
    clip, a later one as the right clip (a script of nothing but one 'S' run does not say which end it is)"""
    a_, b_, g_, _ = wts
    i, j, edits, score, cl, cr = 0, t_begin, 0, 0, 0, 0
    for k, (ln, c) in enumerate(runs):
        if c == "S":
            assert k in (0, len(runs) - 1) and ln > 0
            if k == 0:
                cl = ln
            else:
                cr = ln
            i += ln
        elif c in "=X":
            for _ in range(ln):
                assert (qsym[i] == tsym[j]) == (c == "="), (i, j, c)
                i, j = i + 1, j + 1
            edits += ln if c == "X" else 0
            score += ln * (a_ if c == "=" else -b_)
        elif c == "I":
            i, edits, score = i + ln, edits + ln, score - g_ * ln
        else:
            j, edits, score = j + ln, edits + ln, score - g_ * ln
    return i, j, edits, score, cl, cr


# ---- the map level ----------------------------------------------------------------------------------------------------------------

def rank_candidates(cands, capped, R, wts, T):
    """cands: [(strand, j, edits, chain score, t_begin, t_end, score, clip_left, clip_right)] (status OK only) -> (records, kept count);
    a record is the fields of awry_map_clip_t in their order"""
    a_, b_ = wts[0], wts[1]
    order = sorted((c for c in cands if c[6] >= T), key=lambda c: (-c[6], c[2], c[0], c[4], c[1]))
    kept = []
    for c in order:
        if any(k[0] == c[0] and max(k[4], c[4]) < min(k[5], c[5]) for k in kept):
            continue
        kept.append(c)
    out = []
    for r, (s, j, e, sc, tb, te, score, cl, cr) in enumerate(kept[:R]):
        mapq = 0
        if r == 0 and not capped:
            mapq = MAPQ_MAX if len(kept) < 2 else min(MAPQ_MAX, 10 * (score - kept[1][6]) // (a_ + b_))
        out.append((tb, te, e, sc, j, s, mapq, mp.MAP_SECONDARY if r else 0, score, cl, cr))
    return out, len(kept)


def rank_alignments(aln_off, chains, alns, chain_status, n, A, R, wts, T):
    """the pure ranking over the arrays awry_align_chains_clip_batch returns for the doubled batch of n reads
    -> (map_off uint64[n+1], records MAP_CLIP_NP, per record the index of its alignment, status uint8[n])"""
    off, rows, sel, st = [0], [], [], []
    for i in range(n):
        cands = []
        for s in (0, 1):
            lo, hi = int(aln_off[2 * i + s]), int(aln_off[2 * i + s + 1])
            for j, c in enumerate(range(lo, min(hi, lo + A))):
                if int(alns[c]["status"]) == ca.ALN_OK:
                    cands.append((s, j, int(alns[c]["edits"]), int(chains[c]["score"]), int(alns[c]["t_begin"]), int(alns[c]["t_end"]),
                                  int(alns[c]["score"]), int(alns[c]["clip_left"]), int(alns[c]["clip_right"])))
        capped = mp.Q_SEED_CAP in (int(chain_status[2 * i]), int(chain_status[2 * i + 1]))
        recs, _ = rank_candidates(cands, capped, R, wts, T)
        rows += recs
        sel += [int(aln_off[2 * i + r[5]]) + r[4] for r in recs]
        off.append(off[-1] + len(recs))
        st.append(mp.Q_SEED_CAP if capped else mp.Q_OK)
    return np.array(off, np.uint64), np.array(rows, MAP_CLIP_NP) if rows else np.zeros(0, MAP_CLIP_NP), sel, np.array(st, np.uint8)


def align_queries(tsym, seq_starts, queries, per, A, W, wts, memo=None):
    """tests/chain_ref.py's (status, chains) per query -> per query (status, [(chain, alignment tuple)]) of its first A chains"""
    out = []
    for q, (status, chains) in zip(queries, per):
        qs, rows = None, []
        for c in chains[:A]:
            key = (bytes(q), tuple(c[6]), W, wts[:4])
            if memo is None or key not in memo:
                qs = qs if qs is not None else [int(v) for v in mr.to_symbols(bytes(q), 0)]
                got = align_chain(tsym, seq_starts, qs, list(c[6]), W, wts)
                if memo is not None:
                    memo[key] = got
            else:
                got = memo[key]
            rows.append((c, got))
        out.append((status, rows))
    return out


def map_reads(tsym, seq_starts, reads, chains_of, A, R, W, wts, T, memo=None):
    """chains_of(queries) -> tests/chain_ref.py's [(status, chains)] per query.  -> per read (status, [record], [runs per record])"""
    qs = mp.doubled(reads)
    al = align_queries(tsym, seq_starts, qs, chains_of(qs), A, W, wts, memo)
    out = []
    for i in range(len(reads)):
        cands, runs = [], {}
        for s in (0, 1):
            for j, (c, g) in enumerate(al[2 * i + s][1]):
                if g[0] == ca.ALN_OK:
                    cands.append((s, j, g[3], c[0], g[1], g[2], g[6], g[7], g[8]))
                    runs[(s, j)] = g[4]
        capped = mp.Q_SEED_CAP in (al[2 * i][0], al[2 * i + 1][0])
        recs, _ = rank_candidates(cands, capped, R, wts, T)
        out.append((mp.Q_SEED_CAP if capped else mp.Q_OK, recs, [runs[(r[5], r[4])] for r in recs]))
    return out


def as_csr(per_read):
    """[(status, records, runs)] -> (map_off, records MAP_CLIP_NP, cigar_off, cigar uint32, status)"""
    off, rows, coff, cg, st = [0], [], [0], [np.zeros(0, np.uint32)], []
    for status, recs, runs in per_read:
        st.append(status)
        rows += recs
        for r in runs:
            cg.append(encode(r))
            coff.append(coff[-1] + len(r))
        off.append(off[-1] + len(recs))
    return (np.array(off, np.uint64), np.array(rows, MAP_CLIP_NP) if rows else np.zeros(0, MAP_CLIP_NP), np.array(coff, np.uint64), np.concatenate(cg),
            np.array(st, np.uint8))
