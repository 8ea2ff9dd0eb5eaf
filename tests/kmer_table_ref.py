"""The k-mer count table (awry_amd/csrc/layout.h KT_*, kmer_table.hip.h) as the text defines it -- numpy, no GPU.

The table of a query length L holds every distinct all-ACGT L-mer of the text whose last k letters (k = the seed length) occur
more than 4 times in the text, with its number of occurrences.  A lookup that misses in a line that is not marked overflowed is
answered "count 0" with no search behind it, so the table must hold every such L-mer with exactly its count: reference_table()
recomputes them from sliding windows of the text, expected_lines() says where each must sit and which lines must be marked, and
audit() compares a table read with FmIndex.debug_kmer_table() against that, exactly (the reference determines the table up to
which 16 keys a full line keeps)."""
import numpy as np

KT_CNT_BITS, KT_TAG_SHIFT = 20, 21
KT_TAG_BITS = 64 - KT_TAG_SHIFT
KT_CNT_MASK = (1 << KT_CNT_BITS) - 1
KT_ASK = KT_CNT_MASK
KT_OVERFLOW = 1 << KT_CNT_BITS
KT_TAG_NONE = (1 << KT_TAG_BITS) - 1
LANE_ROWS = 4  # LCX_LANE_ROWS: buckets of up to this many rows are settled in the probe pass and are not in the table

NT_CODE = np.full(256, 8, dtype=np.uint8)
NT_CODE[[65, 67, 71, 84]] = [0, 1, 2, 3]

_U = np.uint64


def kt_mix(words, L):
    """layout.h kt_mix on an array of 2L-bit words: bijective on them (odd multipliers, the high half xored into the low one)"""
    w = np.ascontiguousarray(words, dtype=np.uint64)
    m = _U(0xFFFFFFFFFFFFFFFF) if L >= 32 else _U((1 << (2 * L)) - 1)
    w = (w * _U(0x9E3779B97F4A7C15)) & m  # (uint64 array products wrap)
    w = w ^ (w >> _U(L))
    w = (w * _U(0xD6E8FEB86659FD93)) & m
    w = w ^ (w >> _U(L))
    return w


def pack_queries(q2d):
    """uint8[n, L] of ACGT -> uint64[n], 2 bits per letter, first letter least significant"""
    code = NT_CODE[np.asarray(q2d, dtype=np.uint8)]
    assert (code < 4).all()
    val = np.zeros(len(code), dtype=np.uint64)
    for j in range(code.shape[1]):
        val |= code[:, j].astype(np.uint64) << _U(2 * j)
    return val


def text_windows(text, m):
    """every window text[s .. s + m) -> (uint64 packed as pack_queries, all-ACGT mask), s = 0 .. len(text) - m"""
    code = NT_CODE[np.asarray(text, dtype=np.uint8)]
    n = len(code) - m + 1
    if n <= 0:
        return np.zeros(0, np.uint64), np.zeros(0, bool)
    val = np.zeros(n, dtype=np.uint64)
    ok = np.ones(n, dtype=bool)
    for j in range(m):
        c = code[j:j + n]
        ok &= c < 4
        val |= (c.astype(np.uint64) & _U(3)) << _U(2 * j)
    return val, ok


def kmer_counts(text, m):
    """-> (sorted distinct all-ACGT m-mers of the text, packed; their numbers of occurrences)"""
    val, ok = text_windows(text, m)
    return np.unique(val[ok], return_counts=True)


def reference_table(text, k, L):
    """-> (words uint64, counts int64): every distinct all-ACGT L-mer of the text whose last k letters occur more than LANE_ROWS
    times in the text (every all-ACGT occurrence of the k-mer counts, also one with fewer than L - k letters in front), sorted"""
    assert 0 < k < L <= 32
    words, counts = kmer_counts(text, L)
    kw, kc = kmer_counts(text, k)
    tail = words >> _U(2 * (L - k))  # the last k letters sit in the top bits
    rows = kc[np.searchsorted(kw, tail)]  # (an L-mer's tail occurs, so it is found)
    assert np.array_equal(kw[np.searchsorted(kw, tail)], tail)
    keep = rows > LANE_ROWS
    return words[keep], counts[keep].astype(np.int64)


def expected_lines(words, L, bits):
    """where the keys must sit -> (line of each key, tag of each key, storable mask, storable keys per line, marked mask per line).
    A line is marked iff it has a key whose tag is not storable (>= KT_TAG_NONE) or more than 16 storable keys."""
    mx = kt_mix(words, L)
    line = (mx & _U((1 << bits) - 1)).astype(np.int64)
    tag = mx >> _U(bits)
    storable = tag < _U(KT_TAG_NONE)
    nlines = 1 << bits
    n_store = np.bincount(line[storable], minlength=nlines)
    n_wide = np.bincount(line[~storable], minlength=nlines)
    marked = (n_wide > 0) | (n_store > 16)
    return line, tag, storable, n_store, marked


def audit(table, bits, L, words, counts):
    """asserts that `table` (uint64[16 << bits]) is the table of the reference keys (words, counts) -> (entries, marked lines)"""
    nlines = 1 << bits
    tab = np.asarray(table, dtype=np.uint64).reshape(nlines, 16)
    line, tag, storable, n_store, marked = expected_lines(words, L, bits)
    want_cnt = np.minimum(np.asarray(counts, dtype=np.int64), KT_ASK).astype(np.uint64)
    # the overflow bit: slot 0 of exactly the marked lines, never elsewhere
    ovf = (tab >> _U(KT_CNT_BITS)) & _U(1)
    assert not ovf[:, 1:].any(), ("bit 20 set outside slot 0", np.argwhere(ovf[:, 1:] != 0)[:5])
    got_marked = ovf[:, 0] != 0
    bad = np.flatnonzero(got_marked != marked)
    assert len(bad) == 0, ("overflow marks differ: line, marked, expected, storable keys", [(int(b), bool(got_marked[b]), bool(marked[b]), int(n_store[b])) for b in bad[:5]], len(bad))
    # what is stored: (line, tag) -> count
    s_cnt = tab & _U(KT_CNT_MASK)
    nonempty = s_cnt != 0
    s_line, s_slot = np.nonzero(nonempty)
    s_tag = tab[s_line, s_slot] >> _U(KT_TAG_SHIFT)
    s_cnt = s_cnt[s_line, s_slot]
    assert (s_tag <= (_U(0xFFFFFFFFFFFFFFFF) >> _U(bits))).all() and (s_tag < _U(KT_TAG_NONE)).all(), "a stored tag is wider than any key's"
    s_mx = (s_tag << _U(bits)) | s_line.astype(np.uint64)  # kt_mix is bijective: (line, tag) names the key
    order = np.argsort(s_mx, kind="stable")
    s_mx, s_cnt_sorted = s_mx[order], s_cnt[order]
    assert (s_mx[1:] != s_mx[:-1]).all(), ("a tag appears twice in a line", int(s_line[order][1:][s_mx[1:] == s_mx[:-1]][0]))
    # every stored entry is a reference key of its line with that key's count
    r_mx = (tag[storable] << _U(bits)) | line[storable].astype(np.uint64)
    r_cnt = want_cnt[storable]
    r_order = np.argsort(r_mx, kind="stable")
    r_mx, r_cnt = r_mx[r_order], r_cnt[r_order]
    at = np.searchsorted(r_mx, s_mx)
    known = (at < len(r_mx))
    known[known] = r_mx[at[known]] == s_mx[known]
    assert known.all(), ("entries that are no L-mer of a covered bucket (line, tag, count)",
                         [(int(x & _U(nlines - 1)), int(x >> _U(bits)), int(c)) for x, c in zip(s_mx[~known][:5], s_cnt_sorted[~known][:5])], int((~known).sum()))
    wrong = np.flatnonzero(r_cnt[at] != s_cnt_sorted)
    assert len(wrong) == 0, ("counts differ (line, tag, stored, expected)",
                             [(int(s_mx[j] & _U(nlines - 1)), int(s_mx[j] >> _U(bits)), int(s_cnt_sorted[j]), int(r_cnt[at[j]])) for j in wrong[:5]], len(wrong))
    # every reference key of an unmarked line is stored (exactly once: no tag twice above)
    must = ~marked[line[storable]][r_order]
    found = np.zeros(len(r_mx), dtype=bool)
    found[at] = True
    lost = np.flatnonzero(must & ~found)
    assert len(lost) == 0, ("keys of unmarked lines that are not stored (line, tag, count)",
                            [(int(r_mx[j] & _U(nlines - 1)), int(r_mx[j] >> _U(bits)), int(r_cnt[j])) for j in lost[:5]], len(lost))
    # a marked line is full as far as it can be; with the above: non-empty slots == keys found, nothing else anywhere
    per_line = nonempty.sum(axis=1)
    short = np.flatnonzero(per_line != np.minimum(16, n_store))
    assert len(short) == 0, ("non-empty slots per line differ (line, slots, storable keys)", [(int(b), int(per_line[b]), int(n_store[b])) for b in short[:5]], len(short))
    return int(nonempty.sum()), int(marked.sum())
