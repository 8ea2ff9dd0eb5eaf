"""Two independent references for anchors, the greedy longest-match factorisation of include/awry_hip.h:

(a) definition: the loop of the header run on the canonical text with bytes.find (occurs), bytes.count (count; an
    overlapping search where an anchor can overlap itself) and the oracle's search_range of each anchor substring (rows:
    every anchor occurs, so its rows are canonical) -- for texts up to ~50 kbp;
(b) stepping: the same loop driven through the oracle's initial_search_range / update_range_with_symbol -- no string search
    at all -- for texts of a few Mbp.

Anchors are (q_begin, q_len, start_row, count) tuples in the order found (right to left).  Both map bytes to symbol indices
the way the exact path does (tests/mismatch_ref.py: symbol_lut)."""
import re

import numpy as np

from tests import mismatch_ref as mr


def canonical(x, alphabet):
    """bytes -> the canonical letters of their symbol indices (what the index is built over); rejects what the library rejects"""
    s = mr.to_symbols(x, alphabet)
    if len(s) == 0 or int(s.min()) == 0 or int(s.max()) == 255:
        raise ValueError("empty query, '$' / '#' or a byte >= 0x80")
    return bytes(np.frombuffer(mr.letters(alphabet), np.uint8)[s])


def canonical_text(text, alphabet):
    """the text (ending in '$') as canonical letters"""
    s = mr.to_symbols(bytes(text), alphabet)
    return bytes(np.frombuffer(mr.letters(alphabet), np.uint8)[s])


def _has_border(s):
    return any(s[:j] == s[-j:] for j in range(1, len(s)))


def occurrences(ctext, s):
    """occurrences of s in the canonical text, overlapping ones included"""
    if not _has_border(s):
        return ctext.count(s)
    return len(re.findall(b"(?=" + re.escape(s) + b")", ctext))


def factorise(occurs, L, skip):
    """the header's loop -> [(b, e)] of every anchor, unreported short ones included"""
    out = []
    e = L
    while e > 0:
        if not occurs(e - 1, e):
            e -= 1
            continue
        b = e - 1
        while b > 0 and occurs(b - 1, e):
            b -= 1
        out.append((b, e))
        if b == 0:
            break
        e = b - skip
    return out


def anchors_definition(ctext, oi, query, alphabet, min_len=1, skip=0):
    """reference (a).  ctext: canonical_text(text); oi: the oracle's index of the same text"""
    q = canonical(query, alphabet)
    out = []
    for b, e in factorise(lambda b, e: ctext.find(q[b:e]) >= 0, len(q), skip):
        if e - b < min_len:
            continue
        sp, ep = oi.search_range(q[b:e])
        cnt = occurrences(ctext, q[b:e])
        assert ep - sp + 1 == cnt, (q[b:e], sp, ep, cnt)  # the two sources of (a) agree with each other
        out.append((b, e - b, sp, cnt))
    return out


def anchors_stepping(oi, query, alphabet, min_len=1, skip=0):
    """reference (b): rows by LF steps alone"""
    s = mr.to_symbols(query, alphabet)
    if len(s) == 0 or int(s.min()) == 0 or int(s.max()) == 255:
        raise ValueError("empty query, '$' / '#' or a byte >= 0x80")
    s = [int(v) for v in s]
    out = []
    e = len(s)
    while e > 0:
        sp, ep = oi.initial_search_range(s[e - 1])
        if sp > ep:
            e -= 1
            continue
        b = e - 1
        while b > 0:
            s2, e2 = oi.update_range_with_symbol(sp, ep, s[b - 1])
            if s2 > e2:
                break
            sp, ep, b = s2, e2, b - 1
        if e - b >= min_len:
            out.append((b, e - b, sp, ep - sp + 1))
        if b == 0:
            break
        e = b - skip
    return out


def as_csr(per_query):
    """[[anchor tuples]] -> (anchor_off uint64[n+1], int64[total, 4])"""
    off = np.zeros(len(per_query) + 1, np.uint64)
    off[1:] = np.cumsum([len(a) for a in per_query], dtype=np.uint64)
    flat = [a for aq in per_query for a in aq]
    return off, np.array(flat, np.int64).reshape(-1, 4)


def got_as_rows(anchors):
    """the library's record array -> int64[total, 4] in the column order of the references"""
    return np.stack([anchors[f].astype(np.int64) for f in ("q_begin", "q_len", "start_row", "count")], axis=1).reshape(-1, 4)


def locate_reference(oi, queries, per_query, alphabet, max_hits):
    """-> (hit_off uint64[total+1], global_pos uint64[hits], pos uint64[hits, 2]): the oracle's locate_string of each anchor
    substring with count <= max_hits, concatenated in anchor order"""
    counts, gs, ps = [], [], []
    for q, aq in zip(queries, per_query):
        cq = canonical(q, alphabet)
        for b, ln, _, cnt in aq:
            if cnt > max_hits:
                counts.append(0)
                continue
            g, p = oi.locate_string(cq[b:b + ln])
            assert len(g) == cnt
            counts.append(cnt)
            gs.append(np.asarray(g, np.uint64))
            ps.append(np.array(p, np.uint64).reshape(-1, 2))
    off = np.zeros(len(counts) + 1, np.uint64)
    off[1:] = np.cumsum(counts, dtype=np.uint64)
    g = np.concatenate(gs) if gs else np.zeros(0, np.uint64)
    p = np.concatenate(ps) if ps else np.zeros((0, 2), np.uint64)
    return off, g, p
