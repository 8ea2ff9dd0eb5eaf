"""Reference for the alignment of edit-distance hits (include/awry_hip.h): the definition in numpy / Python over the FULL table,
built on tests/edit_ref.py.

    C[i][j] = edit_distance(q[0..i), T[s..s+j))    0 <= i <= L, 0 <= j <= J = min(L + d, n - s)
    text_len = the smallest j with C[L][j] == d
    traceback from (L, text_len): the diagonal first ('=' / 'X'), then 'I' (i--), then 'D' (j--); reversed and run-length encoded

table(..., band=True) is the same table restricted to |i - j| <= d (cells outside +infinity): what the kernel computes.  Runs are
encoded as the library does, len << 4 | BAM op (I 1, D 2, = 7, X 8)."""
import numpy as np

from tests import edit_ref as er
from tests import mismatch_ref as mr

INF = 1 << 20
MAX_OPS = 17
OP_CODE = {"I": 1, "D": 2, "=": 7, "X": 8}
OP_CHAR = {v: c for c, v in OP_CODE.items()}


def table(tsym, qsym, s, d, band=False):
    """-> int64[L + 1, J + 1]"""
    L, n = len(qsym), len(tsym)
    J = min(L + d, n - s)
    w = np.asarray(tsym[s:s + J], np.int64)
    q = np.asarray(qsym, np.int64)
    idx = np.arange(J + 1, dtype=np.int64)
    C = np.empty((L + 1, J + 1), np.int64)
    C[0] = idx
    if band:
        C[0][idx > d] = INF
    for i in range(1, L + 1):
        tmp = C[i - 1] + 1                                            # 'I'
        np.minimum(tmp[1:], C[i - 1][:-1] + (w != q[i - 1]), out=tmp[1:])  # the diagonal
        if band:
            tmp[np.abs(idx - i) > d] = INF
        row = np.minimum.accumulate(tmp - idx) + idx                  # 'D': the dependency inside the row
        if band:
            row[np.abs(idx - i) > d] = INF
        C[i] = np.minimum(row, INF)
    return C


def script(C, tsym, qsym, s, d):
    """the canonical script of the hit whose table is C -> (text_len, [(length, op letter)] in query order), or None where the
    minimum of row L inside |L - j| <= d is not d (no alignment at that distance)"""
    L, J = C.shape[0] - 1, C.shape[1] - 1
    lo, hi = max(L - d, 0), min(L + d, J)
    if hi < lo or int(C[L][lo:hi + 1].min()) != d:
        return None
    j = lo + int(np.nonzero(C[L][lo:hi + 1] == d)[0][0])
    text_len, i, ops = j, L, []
    while i or j:
        if i and j and C[i - 1][j - 1] + (qsym[i - 1] != tsym[s + j - 1]) == C[i][j]:
            ops.append("=" if qsym[i - 1] == tsym[s + j - 1] else "X")
            i, j = i - 1, j - 1
        elif i and C[i - 1][j] + 1 == C[i][j]:
            ops.append("I")
            i -= 1
        else:
            assert j and C[i][j - 1] + 1 == C[i][j]
            ops.append("D")
            j -= 1
    runs = []
    for c in reversed(ops):
        if runs and runs[-1][1] == c:
            runs[-1][0] += 1
        else:
            runs.append([1, c])
    return text_len, [(ln, c) for ln, c in runs]


def encode(runs):
    return np.array([ln << 4 | OP_CODE[c] for ln, c in runs], np.uint32)


def cigar_text(runs):
    return "".join("%d%s" % (ln, c) for ln, c in runs)


def align_triple(t, query, s, d, band=False):
    """one triple on an edit_ref.Text -> (text_len, uint32 runs); (0, no runs) for a triple that is no alignment at that distance"""
    q = mr.to_symbols(bytes(query), t.alphabet)
    if s >= t.n or not len(q):
        return 0, np.zeros(0, np.uint32)
    got = script(table(t.sym, q, s, d, band), t.sym, q, s, d)
    if got is None:
        return 0, np.zeros(0, np.uint32)
    return got[0], encode(got[1])


def align_many(t, query, starts, dists):
    """the hits (query, starts[h], dists[h]) of one query on an edit_ref.Text, all tables at once -> (text_len uint32[H], [uint32
    runs] per hit).  The same definition as table() / script(), vectorised over the hits (a 9-mer within 8 edits has thousands):
    every table gets L + max(dists) columns over a text padded past its end -- cells right of a hit's own J never feed a cell
    left of them, and the traceback only moves left."""
    q = np.asarray(mr.to_symbols(bytes(query), t.alphabet), np.int64)
    L, H = len(q), len(starts)
    S, D = np.asarray(starts, np.int64), np.asarray(dists, np.int64)
    tls, runs = np.zeros(H, np.uint32), [None] * H
    if not H:
        return tls, runs
    Jm = L + int(D.max())
    pad = np.concatenate([np.asarray(t.sym, np.int64), np.full(Jm + 1, -1, np.int64)])
    idx = np.arange(Jm + 1, dtype=np.int64)
    step = max(1, 20_000_000 // ((L + 1) * (Jm + 1)))
    for lo in range(0, H, step):
        s, d = S[lo:lo + step], D[lo:lo + step]
        h = np.arange(len(s))
        W = pad[s[:, None] + idx[None, :Jm]]
        C = np.empty((len(s), L + 1, Jm + 1), np.int64)
        C[:, 0, :] = idx
        for i in range(1, L + 1):
            tmp = C[:, i - 1, :] + 1
            np.minimum(tmp[:, 1:], C[:, i - 1, :-1] + (W != q[i - 1]), out=tmp[:, 1:])
            C[:, i, :] = np.minimum.accumulate(tmp - idx, axis=1) + idx
        J = np.minimum(L + d, t.n - s)
        ok = (C[:, L, :] == d[:, None]) & (idx[None, :] <= J[:, None])
        assert ok.any(axis=1).all() and (np.where(idx[None, :] <= J[:, None], C[:, L, :], INF).min(axis=1) == d).all()
        j = ok.argmax(axis=1)
        tls[lo:lo + step] = j
        i = np.full(len(s), L, np.int64)
        ops = np.zeros((len(s), L + Jm), np.uint8)
        for x in range(L + Jm):
            live = (i > 0) | (j > 0)
            if not live.any():
                break
            i1, j1 = np.maximum(i - 1, 0), np.maximum(j - 1, 0)
            here = C[h, i, j]
            neq = q[i1] != pad[s + j1]
            diag = live & (i > 0) & (j > 0) & (C[h, i1, j1] + neq == here)
            up = live & ~diag & (i > 0) & (C[h, i1, j] + 1 == here)
            left = live & ~diag & ~up
            assert (~left | ((j > 0) & (C[h, i, j1] + 1 == here))).all()
            ops[:, x] = np.where(diag, np.where(neq, OP_CODE["X"], OP_CODE["="]), np.where(up, OP_CODE["I"], np.where(left, OP_CODE["D"], 0)))
            i = i - (diag | up)
            j = j - (diag | left)
        for a in h:
            o = ops[a][ops[a] != 0][::-1].astype(np.int64)
            cut = np.concatenate([[0], np.nonzero(np.diff(o))[0] + 1, [len(o)]])
            runs[lo + a] = ((np.diff(cut) << 4) | o[cut[:-1]]).astype(np.uint32)
    return tls, runs


def align(t, queries, k, max_candidates):
    """-> edit_ref.Text.locate's (hit_off, global_pos, edits, status), then text_len uint32[total], cigar_off uint64[total + 1],
    cigar uint32[runs]"""
    off, g, d, st = t.locate(queries, k, max_candidates)
    tls, runs = [], []
    for i, q in enumerate(queries):
        tl, r = align_many(t, q, g[int(off[i]):int(off[i + 1])], d[int(off[i]):int(off[i + 1])])
        tls.append(tl)
        runs += r
    coff = np.zeros(len(g) + 1, np.uint64)
    coff[1:] = np.cumsum([len(r) for r in runs], dtype=np.uint64)
    return (off, g, d, st, np.concatenate(tls) if tls else np.zeros(0, np.uint32), coff,
            np.concatenate(runs) if runs else np.zeros(0, np.uint32))
