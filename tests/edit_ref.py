"""Reference for locate within k edits (include/awry_hip.h): the definition in numpy, over a whole text.

    D(s) = min over e in [s, n] of edit_distance(q, T[s..e))       T = the text without '$', D(-1) = D(n) = +inf
    s is a hit with distance D(s)  iff  D(s) <= k  and  D(s-1) >= D(s)  and  D(s+1) >= D(s)

distances() fills the table row by row from the query's last letter: C_i[s] = min over e of edit_distance(q[i..], T[s..e)),
C_L = 0, and C_i[s] = min(C_{i+1}[s] + 1, C_{i+1}[s+1] + (q[i] != T[s]), C_i[s+1] + 1).  The last term is the dependency inside a
row; it is resolved by a running minimum of (value + index) from the right.  L row updates over vectors of the text's length.

The piece / candidate-cap rule runs on the canonical text with string search (tests/anchor_ref.py).  window_pipeline() is the
device's plan in Python -- pieces, diagonals, merged runs, cut windows -- for the CPU check that it equals the global rule.
Bytes are mapped to symbol indices as on the exact path (tests/mismatch_ref.py)."""
import re

import numpy as np

from tests import anchor_ref as ar
from tests import mismatch_ref as mr

Q_CANDIDATE_CAP = 7
INF = 1 << 30


def distances(tsym, qsym):
    """tsym: symbol indices of T (no '$'), qsym: of the query -> int32[n], D(s) for every start"""
    n, L = len(tsym), len(qsym)
    idx = np.arange(n + 1, dtype=np.int32)
    row = np.zeros(n + 1, np.int32)  # C_L
    tmp = np.empty(n + 1, np.int32)
    for i in range(L - 1, -1, -1):
        tmp[:] = row + 1
        np.minimum(tmp[:n], row[1:] + (tsym != qsym[i]), out=tmp[:n])
        row = np.minimum.accumulate((tmp + idx)[::-1])[::-1] - idx
    return row[:n].astype(np.int32)


def hits_of(D, k, lo=0, hi=None):
    """the hit rule over D (whole text) -> (positions int64[], distances uint8[]) ascending; lo / hi restrict the starts reported"""
    n = len(D)
    hi = n if hi is None else hi
    P = np.full(n + 2, INF, np.int64)
    P[1:n + 1] = D
    ok = (P[1:-1] <= k) & (P[:-2] >= P[1:-1]) & (P[2:] >= P[1:-1])
    pos = np.nonzero(ok)[0]
    pos = pos[(pos >= lo) & (pos < hi)]
    return pos.astype(np.int64), D[pos].astype(np.uint8)


def pieces(L, k):
    """[(begin, end)] of the k + 1 pieces of a query of L letters"""
    return [(t * L // (k + 1), (t + 1) * L // (k + 1)) for t in range(k + 1)]


def find_all(ctext, s):
    """every occurrence of s in the canonical text, overlapping ones included, ascending"""
    return [m.start() for m in re.finditer(b"(?=" + re.escape(s) + b")", ctext)]


def candidates(ctext, query, k, alphabet):
    """c(q): the sum of the exact occurrence counts of the k + 1 pieces"""
    cq = ar.canonical(query, alphabet)
    return sum(ar.occurrences(ctext, cq[b:e]) for b, e in pieces(len(cq), k))


class Text:
    """a text (ending in '$') prepared for the reference: symbol indices without the sentinel, and the canonical letters"""

    def __init__(self, text, alphabet):
        self.alphabet = alphabet
        self.sym = mr.to_symbols(bytes(text), alphabet)[:-1]
        self.ctext = ar.canonical_text(text, alphabet)
        self.n = len(self.sym)
        self._D = {}

    def D(self, query):
        key = bytes(query)
        if key not in self._D:
            q = mr.to_symbols(key, self.alphabet)
            assert len(q) and int(q.min()) > 0 and int(q.max()) != 255
            self._D[key] = distances(self.sym, q)
        return self._D[key]

    def locate(self, queries, k, max_candidates):
        """-> (hit_off uint64[n+1], global_pos uint64[], edits uint8[], status uint8[n]) of the contract"""
        counts, gs, ds, st = [], [], [], []
        for q in queries:
            assert k < len(q) <= 256
            if candidates(self.ctext, q, k, self.alphabet) > max_candidates:
                counts.append(0)
                st.append(Q_CANDIDATE_CAP)
                continue
            p, d = hits_of(self.D(q), k)
            counts.append(len(p))
            gs.append(p.astype(np.uint64))
            ds.append(d)
            st.append(0)
        off = np.zeros(len(queries) + 1, np.uint64)
        off[1:] = np.cumsum(counts, dtype=np.uint64)
        g = np.concatenate(gs) if gs else np.zeros(0, np.uint64)
        d = np.concatenate(ds) if ds else np.zeros(0, np.uint8)
        return off, g, d, np.array(st, np.uint8)


def windows_of(ctext, n, query, k, alphabet):
    """the plan's windows of one query: [(first, count)] of owned starts, ascending and disjoint"""
    cq = ar.canonical(query, alphabet)
    L = len(cq)
    diags = sorted(set(g - b for b, e in pieces(L, k) for g in find_all(ctext, cq[b:e])))
    runs = []
    for d in diags:
        if runs and d - runs[-1][1] <= 2 * k + 1:
            runs[-1][1] = d
        else:
            runs.append([d, d])
    out = []
    for lo, hi in runs:
        first, last = max(lo - k, 0), min(hi + k, n - 1)
        if last >= first:
            out.append((first, last - first + 1))
    return out


def scanned(first, count, L, k, n):
    """the text a window's scan reads: [a, b)"""
    return max(first - 1, 0), min(first + count - 1 + L + k + 3, n)


def window_hits(tsym, qsym, k, first, count):
    """the hit rule for the owned starts of one window, from the cut text alone"""
    n, L = len(tsym), len(qsym)
    a, b = scanned(first, count, L, k, n)
    D = distances(tsym[a:b], qsym).astype(np.int64)
    P = np.full(b - a + 2, INF, np.int64)  # P[j + 1] = D(a + j); what lies outside the scan is +inf: only the text's two ends are ever asked for
    P[1:-1] = D
    out = []
    for s in range(first, min(first + count, n)):
        j = s - a + 1
        if P[j] <= k and P[j - 1] >= P[j] and P[j + 1] >= P[j]:
            out.append((s, int(P[j])))
    return out


def window_pipeline(t, query, k):
    """the device's plan for one query on a Text -> [(position, distance)] ascending"""
    q = mr.to_symbols(bytes(query), t.alphabet)
    out = []
    for first, count in windows_of(t.ctext, t.n, query, k, t.alphabet):
        if first > 0:
            assert scanned(first, count, len(q), k, t.n)[0] == first - 1
        out += window_hits(t.sym, q, k, first, count)
    return out
