"""Reference for the alignment of chains (include/awry_hip.h, "align chains"): the definition in plain Python integers, stated
twice.

A chain's members (q_begin, q_len, t_pos), in their reported order, are clipped into pieces that overlap neither in the query nor in
the text; a piece is a diagonal run ('=' / 'X' letter by letter).  The query before the first piece, between consecutive pieces and
after the last is aligned by segments -- a left extension (on reversed strings), gaps (global) and a right extension -- inside the
band lo <= j - i <= hi, lo = min(0, m) - W, hi = max(0, m) + W.  The traceback of every segment takes the diagonal first, then 'I'
(i--), then 'D' (j--), on banded values.

segment(..., full=False) keeps one row of hi - lo + 1 cells and a direction per cell, as the kernel does; full=True fills the whole
(a + 1) x (J + 1) table with the band as a condition on cells and traces back by comparing values.  unbanded() is the plain table
the header's properties are stated against.  Runs are encoded as the library does, len << 4 | BAM op (I 1, D 2, = 7, X 8)."""
import numpy as np

INF = 1 << 20
MAX_BAND, MAX_SKEW, MAX_LEN = 8, 16, 1024
ALN_OK, ALN_SKEW, ALN_BAD_CHAIN = 0, 1, 2
OP_CODE = {"I": 1, "D": 2, "=": 7, "X": 8}
OP_CHAR = {v: c for c, v in OP_CODE.items()}


def band_of(m, W):
    return min(0, m) - W, max(0, m) + W


def cells_of(a, J, m, W):
    """table cells inside band and table: (i, j), 0 <= i <= a, 0 <= j <= J, lo <= j - i <= hi"""
    lo, hi = band_of(m, W)
    return sum(max(0, min(J, i + hi) - max(0, i + lo) + 1) for i in range(a + 1))


def _banded(x, y, J, m, W, end):
    a = len(x)
    lo, hi = band_of(m, W)
    NB = hi - lo + 1
    c = [b + lo if 0 <= b + lo <= J else INF for b in range(NB)]  # row 0
    dirs = [None]
    for i in range(1, a + 1):
        new, d, left = [INF] * NB, [3] * NB, INF
        for b in range(NB):
            j = i + b + lo
            if j < 0 or j > J:
                left = INF
                continue
            if j == 0:
                v, dr = i, 2  # column 0: only 'I' leads back
            else:
                neq = int(x[i - 1] != y[j - 1])
                dg, up, lf = c[b] + neq, (c[b + 1] if b + 1 < NB else INF) + 1, left + 1
                v = min(dg, up, lf)
                dr = neq if dg == v else 2 if up == v else 3
            new[b], d[b], left = v, dr, v
        c = new
        dirs.append(d)
    if end is None:
        cost = min(c)
        b = c.index(cost)  # the first minimum: the smallest end column
    else:
        b = end - a - lo
        cost = c[b]
    assert cost < INF
    i, j, ops = a, a + b + lo, []
    jstar = j
    while i or j:
        dr = dirs[i][j - i - lo] if i else 3  # row 0: only 'D' leads back
        ops.append("=XID"[dr])
        if dr <= 1:
            i, j = i - 1, j - 1
        elif dr == 2:
            i -= 1
        else:
            j -= 1
        assert j >= 0 and (i == 0 and j == 0 or lo <= j - i <= hi)
    return cost, jstar, ops


def _table(x, y, J, band):
    """C[i][j], 0 <= i <= len(x), 0 <= j <= J; band = (lo, hi) or None for the unbanded table"""
    a = len(x)
    C = [[INF] * (J + 1) for _ in range(a + 1)]
    for i in range(a + 1):
        for j in range(J + 1):
            if band is not None and not band[0] <= j - i <= band[1]:
                continue
            if i == 0 and j == 0:
                C[i][j] = 0
                continue
            v = INF
            if i and j:
                v = min(v, C[i - 1][j - 1] + int(x[i - 1] != y[j - 1]))
            if i:
                v = min(v, C[i - 1][j] + 1)
            if j:
                v = min(v, C[i][j - 1] + 1)
            C[i][j] = min(v, INF)
    return C


def _full(x, y, J, m, W, end):
    a = len(x)
    C = _table(x, y, J, band_of(m, W))
    if end is None:
        cost = min(C[a])
        j = C[a].index(cost)
    else:
        j, cost = end, C[a][end]
    assert cost < INF
    i, jstar, ops = a, j, []
    while i or j:
        if i and j and C[i - 1][j - 1] + int(x[i - 1] != y[j - 1]) == C[i][j]:
            ops.append("=" if x[i - 1] == y[j - 1] else "X")
            i, j = i - 1, j - 1
        elif i and C[i - 1][j] + 1 == C[i][j]:
            ops.append("I")
            i -= 1
        else:
            assert j and C[i][j - 1] + 1 == C[i][j]
            ops.append("D")
            j -= 1
    return cost, jstar, ops


def unbanded(x, y, J):
    return _table(x, y, J, None)


def segment(x, y, J, m, W, end=None, full=False):
    """x (a symbols) against the prefixes of y[0..J) -> (cost, end column, operations from (a, end) back to (0, 0)); end = None:
    the smallest column that minimises row a"""
    return (_full if full else _banded)(list(x), list(y), J, m, W, end)


def pieces_of(members, L, n):
    """-> (status, [(qb, len, tp)]): ALN_BAD_CHAIN for an empty list, a member past L or n, or members not strictly ascending in
    both q_begin and t_pos"""
    if not members or L < 1 or L > MAX_LEN:
        return ALN_BAD_CHAIN, []
    for k, (qb, ln, tp) in enumerate(members):
        if qb + ln > L or tp + ln > n:
            return ALN_BAD_CHAIN, []
        if k and not (qb > members[k - 1][0] and tp > members[k - 1][2]):
            return ALN_BAD_CHAIN, []
    qb, ln, tp = members[0]
    out, qe, te = [(qb, ln, tp)], qb + ln, tp + ln
    for qb, ln, tp in members[1:]:
        o = max(0, qe - qb, te - tp)
        if o >= ln:
            continue
        out.append((qb + o, ln - o, tp + o))
        qe, te = qb + ln, tp + ln
    return ALN_OK, out


def rle(ops):
    runs = []
    for c in ops:
        if runs and runs[-1][1] == c:
            runs[-1][0] += 1
        else:
            runs.append([1, c])
    return [(ln, c) for ln, c in runs]


def encode(runs):
    return np.array([ln << 4 | OP_CODE[c] for ln, c in runs], np.uint32)


def cigar_text(runs):
    return "".join("%d%s" % (ln, c) for ln, c in runs)


def align_chain(tsym, qsym, members, W, full=False):
    """-> (status, t_begin, t_end, edits, [(length, op letter)], table cells) of one chain on the text's symbol indices"""
    n, L = len(tsym), len(qsym)
    status, pcs = pieces_of(members, L, n)
    if status:
        return status, 0, 0, 0, [], 0
    tb, te = pcs[0][2], pcs[-1][2] + pcs[-1][1]
    qb0, qe_last = pcs[0][0], pcs[-1][0] + pcs[-1][1]
    left_m, right_m = min(0, tb - qb0), min(0, (n - te) - (L - qe_last))
    skews = [left_m, right_m]
    for (q0, l0, t0), (q1, _, t1) in zip(pcs, pcs[1:]):
        skews.append((t1 - (t0 + l0)) - (q1 - (q0 + l0)))
    if max(abs(m) for m in skews) > MAX_SKEW:
        return ALN_SKEW, tb, te, 0, [], 0
    ops, edits, cells = [], 0, 0
    t_begin, t_end = tb, te
    if qb0:
        a, avail = qb0, tb
        J = min(a + W, avail)
        x = [qsym[qb0 - 1 - i] for i in range(a)]
        y = [tsym[tb - 1 - j] for j in range(J)]
        cost, jstar, sops = segment(x, y, J, left_m, W, None, full)
        ops += sops  # reversed strings: the traceback's order is the query's
        edits += cost
        cells += cells_of(a, J, left_m, W)
        t_begin = tb - jstar
    for k, (qb, ln, tp) in enumerate(pcs):
        if k:
            q0, t0 = pcs[k - 1][0] + pcs[k - 1][1], pcs[k - 1][2] + pcs[k - 1][1]
            a, b = qb - q0, tp - t0
            cost, _, sops = segment(qsym[q0:qb], tsym[t0:tp], b, b - a, W, b, full)
            ops += sops[::-1]
            edits += cost
            cells += cells_of(a, b, b - a, W)
        for i in range(ln):
            neq = qsym[qb + i] != tsym[tp + i]
            ops.append("X" if neq else "=")
            edits += int(neq)
    if qe_last < L:
        a, avail = L - qe_last, n - te
        J = min(a + W, avail)
        cost, jstar, sops = segment(qsym[qe_last:], tsym[te:te + J], J, right_m, W, None, full)
        ops += sops[::-1]
        edits += cost
        cells += cells_of(a, J, right_m, W)
        t_end = te + jstar
    return ALN_OK, t_begin, t_end, edits, rle(ops), cells


def widest_band(tsym_len, L, members, W):
    """NB = |m| + 2 W + 1 of the chain's widest segment (what the kernel's classes are cut by); None for a chain not aligned"""
    status, pcs = pieces_of(members, L, tsym_len)
    if status:
        return None
    skews = [min(0, pcs[0][2] - pcs[0][0]), min(0, (tsym_len - pcs[-1][2] - pcs[-1][1]) - (L - pcs[-1][0] - pcs[-1][1]))]
    for (q0, l0, t0), (q1, _, t1) in zip(pcs, pcs[1:]):
        skews.append((t1 - (t0 + l0)) - (q1 - (q0 + l0)))
    m = max(abs(x) for x in skews)
    return None if m > MAX_SKEW else m + 2 * W + 1


def replay(qsym, tsym, t_begin, runs):
    """walk the script over q and T[t_begin ..) -> (query letters consumed, text end, edits); asserts '=' / 'X' letter by letter"""
    i, j, edits = 0, t_begin, 0
    for ln, c in runs:
        if c in "=X":
            for _ in range(ln):
                assert (qsym[i] == tsym[j]) == (c == "="), (i, j, c)
                i, j = i + 1, j + 1
            edits += ln if c == "X" else 0
        elif c == "I":
            i, edits = i + ln, edits + ln
        else:
            j, edits = j + ln, edits + ln
    return i, j, edits


ALN_NP = np.dtype([("t_begin", "<u8"), ("t_end", "<u8"), ("edits", "<u4"), ("status", "<u4")])
