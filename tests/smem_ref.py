"""Two independent references for SMEMs, the super-maximal exact matches of include/awry_hip.h:

(a) definition: occurs(b, e) by bytes.find on the canonical text; rows from the oracle's search_range of each SMEM substring,
    cross-checked against an overlapping occurrence count as tests/anchor_ref.py does -- for texts up to ~50 kbp;
(b) oracle: occurs(b, e) by the oracle's count_string, rows by its search_range -- no string search, for texts of a few Mbp.

Both run the same two-pointer over the end e: b(e) = the smallest b with occurs(b, e) (b(e) = e when the letter e-1 is absent)
does not decrease with e, so it is found by moving b right from b(e-1); (b(e), e) is left-maximal by construction and is
right-maximal exactly when e == L or b(e+1) > b(e).  Neither uses the library's right-to-left algorithm.

SMEMs are (q_begin, q_len, start_row, count) tuples in descending q_begin, the order of the library."""
from tests import anchor_ref as ar


def maximal_pairs(occurs, L):
    """-> [(b, e)] of every SMEM, ascending"""
    bs = []
    b = 0
    for e in range(1, L + 1):
        while b < e and not occurs(b, e):
            b += 1
        bs.append(b)
    return [(bs[e - 1], e) for e in range(1, L + 1) if bs[e - 1] < e and (e == L or bs[e] > bs[e - 1])]


def is_smem(occurs, L, b, e):
    """the three conditions of the header, literally"""
    return 0 <= b < e <= L and occurs(b, e) and (b == 0 or not occurs(b - 1, e)) and (e == L or not occurs(b, e + 1))


def smems_definition(ctext, oi, query, alphabet, min_len=1):
    """reference (a).  ctext: anchor_ref.canonical_text(text); oi: the oracle's index of the same text"""
    q = ar.canonical(query, alphabet)
    out = []
    for b, e in reversed(maximal_pairs(lambda b, e: ctext.find(q[b:e]) >= 0, len(q))):
        if e - b < min_len:
            continue
        sp, ep = oi.search_range(q[b:e])
        cnt = ar.occurrences(ctext, q[b:e])
        assert ep - sp + 1 == cnt, (q[b:e], sp, ep, cnt)  # the two sources of (a) agree with each other
        out.append((b, e - b, sp, cnt))
    return out


def smems_oracle(oi, query, alphabet, min_len=1):
    """reference (b): the oracle's count_string / search_range alone"""
    q = ar.canonical(query, alphabet)
    memo = {}

    def occurs(b, e):
        if (b, e) not in memo:
            memo[(b, e)] = oi.count_string(q[b:e]) > 0
        return memo[(b, e)]

    out = []
    for b, e in reversed(maximal_pairs(occurs, len(q))):
        if e - b < min_len:
            continue
        sp, ep = oi.search_range(q[b:e])
        assert ep - sp + 1 == oi.count_string(q[b:e])
        out.append((b, e - b, sp, ep - sp + 1))
    return out
