"""Locate within k edits on the GPU (awry_amd/csrc/edit_kernels.hip.h, edit_host.h) against the definition in tests/edit_ref.py:
positions, distances, order, offsets and status, for exact equality.  Wherever the comparison is with the reference,
max_candidates is large enough that no query is abandoned, and the test asserts that the status bytes say so.  Results must not
depend on the accelerators, the seed table, the chunk capacity or the number of replicas."""
import os

import numpy as np
import pytest

import awry_amd
from awry_amd.fm_index import ERR_ARG, ERR_INVALID_QUERY, Q_CANDIDATE_CAP, AwryError, FmIndex, pack_queries
from tests import edit_ref as er
from tests import synth

pytestmark = pytest.mark.gpu

NO_CAP = 10 ** 9
LENGTHS = (20, 63, 64, 65, 101, 127, 128, 129, 192, 193, 255, 256)


class World:
    def __init__(self, text, st, hd, alphabet):
        self.text, self.st, self.alphabet = text, np.array(st, np.uint64), alphabet
        self.ix = FmIndex.from_text(text, alphabet, 8, 0, st, hd).set_devices([0])
        self.t = er.Text(text, alphabet)
        self.n = self.t.n
        self.letters = synth.NT if alphabet == 0 else synth.AA


def check(w, qs, k, ix=None, max_candidates=NO_CAP):
    """one batch call against the reference; -> the library's arrays"""
    ix = w.ix if ix is None else ix
    off, g, p, d, st = ix.parallel_locate_edit_csr(*pack_queries(qs), k, max_candidates)
    woff, wg, wd, wst = w.t.locate(qs, k, max_candidates)
    assert st.dtype == np.uint8 and np.array_equal(st, wst)
    if max_candidates == NO_CAP:
        assert not st.any()
    assert np.array_equal(off, woff), (k, [len(q) for q in qs])
    assert np.array_equal(g, wg)
    assert np.array_equal(d, wd)
    for i in range(len(qs)):  # strictly ascending positions: no start is reported twice
        assert np.all(np.diff(g[off[i]:off[i + 1]].astype(np.int64)) > 0)
    rec = np.searchsorted(w.st, g, side="right") - 1
    assert np.array_equal(p[:, 0], rec.astype(np.uint64)) and np.array_equal(p[:, 1], g - w.st[rec])
    return off, g, p, d, st


def other(letters, c):
    i = np.nonzero(letters == c)[0]
    return int(letters[(int(i[0]) + 1) % len(letters)]) if len(i) else int(letters[0])


def planted(w, rng, L, ops, p=None):
    """a read of exactly L letters: the text at p with the edits `ops` = [(kind, position in the read)], kind 's' / 'i' / 'd';
    -> (read, p).  Positions are applied from the right, so each is a position of the source window."""
    src = L - sum(1 for o in ops if o[0] == "i") + sum(1 for o in ops if o[0] == "d")
    assert src >= 1
    if p is None:
        p = int(rng.integers(0, w.n - src))
    q = bytearray(w.text[p:p + src])
    for kind, j in sorted(ops, key=lambda o: -o[1]):
        j = min(j, len(q) - 1)
        if kind == "s":
            q[j] = other(w.letters, q[j])
        elif kind == "i":
            q.insert(j, other(w.letters, q[j]))
        else:
            del q[j]
    assert len(q) == L, (L, ops)
    return bytes(q), p


def random_ops(rng, L, e):
    pos = rng.choice(L - 1, size=min(e, L - 1), replace=False) if L > 1 else []
    return [("sid"[int(rng.integers(0, 3))], int(j)) for j in pos]


def reads_for(w, rng, L, k):
    """reads of L letters with 0 .. k + 1 planted edits of each kind, edits in the first and last two letters, edits that
    straddle a piece boundary, and k + 1 spread substitutions; -> (reads, [(read index, locus)] of the last kind)"""
    qs, far = [], []
    for e in range(0, k + 2):
        if e < L:
            qs.append(planted(w, rng, L, random_ops(rng, L, e))[0])
    if L >= 8:
        for ops in ([("s", 0)], [("d", 1)], [("i", L - 2)], [("s", L - 2), ("s", 1)], [("i", 0), ("d", L - 1)]):
            qs.append(planted(w, rng, L, ops)[0])
        b1 = L // (k + 1)  # where piece 1 begins
        if k >= 1 and 1 <= b1 < L - 1:
            qs.append(planted(w, rng, L, [("s", b1 - 1), ("i", b1)])[0])
            qs.append(planted(w, rng, L, [("d", b1)])[0])
    if L >= 63:
        q, p = planted(w, rng, L, [("s", int(j)) for j in np.linspace(1, L - 2, k + 1).astype(int)])
        far.append((len(qs), p))
        qs.append(q)
    return qs, far


@pytest.fixture(scope="module")
def nt():
    return World(*synth.make_text(20_000, 0, 51, 5, 0.01), 0)


@pytest.mark.parametrize("k", [0, 1, 2, 3, 5, 8])
def test_planted_edits_at_every_word_edge(nt, k):
    rng = np.random.default_rng(100 + k)
    groups = {}  # words per column -> reads: one call per W, so that every instantiation of the scan runs
    for L in sorted(set((k + 1, 2 * (k + 1)) + LENGTHS)):
        qs, far = reads_for(nt, rng, L, k)
        g = groups.setdefault((L + 63) // 64, ([], []))
        g[1].extend((len(g[0]) + i, p) for i, p in far)
        g[0].extend(qs)
    assert sorted(groups) == [1, 2, 3, 4]
    total = 0
    for W, (qs, far) in sorted(groups.items()):
        off, g, _, d, _ = check(nt, qs, k)
        total += len(g)
        for i, p in far:  # k + 1 edits: no hit from that locus
            hits = g[off[i]:off[i + 1]].astype(np.int64)
            assert not np.any(np.abs(hits - p) <= k + 1), (W, i, p)
    assert total > 20


def test_mixed_lengths_in_one_call(nt):
    rng = np.random.default_rng(7)
    qs = []
    for L in (3, 6, 20, 63, 64, 65, 101, 128, 129, 192, 193, 256):
        qs += reads_for(nt, rng, L, 2)[0][:4]
    order = rng.permutation(len(qs))
    check(nt, [qs[i] for i in order], 2)


def test_k0_equals_exact_locate(nt):
    rng = np.random.default_rng(8)
    qs = [bytes(nt.text[p:p + L]) for L in (1, 2, 8, 31, 64, 101, 200) for p in rng.integers(0, nt.n - 200, size=5)] + [b"N", b"NN", b"ACGTTGCAAC"]
    qb, qo = pack_queries(qs)
    off, g, _, d, st = nt.ix.parallel_locate_edit_csr(qb, qo, 0, NO_CAP)
    xoff, xg, _ = nt.ix.parallel_locate_csr(qb, qo)
    assert np.array_equal(off, xoff) and not d.any() and not st.any()
    for i in range(len(qs)):
        assert np.array_equal(g[off[i]:off[i + 1]], np.sort(xg[xoff[i]:xoff[i + 1]])), qs[i]
    check(nt, qs, 0)


def test_mismatch_hits_bound_the_reference(nt):
    """an existing path checks the reference: a hit of the substitution search at distance d has D <= d"""
    rng = np.random.default_rng(9)
    qs = [planted(nt, rng, L, [("s", int(j)) for j in rng.choice(L, size=e, replace=False)])[0] for L in (24, 40, 101) for e in (0, 1, 2) for _ in range(2)]
    off, g, _, d = nt.ix.parallel_locate_mismatch_csr(*pack_queries(qs), 2)
    assert len(g) >= len(qs)
    for i, q in enumerate(qs):
        D = nt.t.D(q)
        assert np.all(D[g[off[i]:off[i + 1]].astype(np.int64)] <= d[off[i]:off[i + 1]]), q


@pytest.fixture(scope="module")
def runs():
    """a one-record text without N: a homopolymer and tandem arrays of period 2 and 3 between random flanks"""
    rng = np.random.default_rng(52)
    rnd = lambda m: bytes(synth.NT[rng.integers(0, 4, size=m)])
    body = rnd(300) + b"A" * 200 + b"CT" + b"AC" * 120 + b"GG" + b"ACG" * 90 + rnd(300) + b"T" * 90
    text = np.frombuffer(body + b"$", np.uint8).copy()
    return World(text, [0], ["r0"], 0)


@pytest.mark.parametrize("k", [1, 2, 3])
def test_homopolymer_and_tandem_arrays(runs, k):
    qs = [b"A" * 30, b"A" * 70, b"A" * 35 + b"C" + b"A" * 34, b"AC" * 20, b"AC" * 10 + b"A" + b"AC" * 10, b"ACG" * 15, b"ACG" * 7 + b"AG" + b"ACG" * 7,
          b"CA" * 33, b"T" * 64, b"T" * 100, b"GT" + b"A" * 63, b"A" * 199 + b"CT", b"A" * 210]
    off, g, _, d, _ = check(runs, qs, k)
    counts = np.diff(off.astype(np.int64))
    assert counts[0] > 100 and counts[3] > 50 and counts[5] > 50  # plateaus are reported whole, through merged windows


@pytest.mark.parametrize("k", [2, 3])
def test_text_ends_and_overhanging_reads(nt, k):
    rng = np.random.default_rng(10 + k)
    rnd = lambda m: bytes(synth.NT[rng.integers(0, 4, size=m)])
    n, text = nt.n, nt.text
    qs = [bytes(text[:40]), bytes(text[1:41]), rnd(2) + bytes(text[:40]), rnd(k) + bytes(text[:64]), rnd(k + 1) + bytes(text[:64]),
          bytes(text[n - 40:n]), bytes(text[n - 41:n - 1]), bytes(text[n - 40:n]) + rnd(2), bytes(text[n - 64:n]) + rnd(k), bytes(text[n - 64:n]) + rnd(k + 1),
          bytes(text[n - 3:n]) + b"A", bytes(text[:k + 1])]
    off, g, _, d, _ = check(nt, qs, k)
    assert g[off[0]] == 0 and g[off[2]] == 0 and int(g[off[6] - 1]) == n - 40  # a hit at start 0; a window that ends at n


@pytest.mark.parametrize("k", [1, 3])
def test_record_joins_and_n_runs(nt, k):
    rng = np.random.default_rng(20 + k)
    text = nt.text
    joins = [int(s) - 1 for s in nt.st[1:]]
    assert all(text[j] == ord("N") for j in joins)
    nruns = np.nonzero((text[:-1] == ord("N")) & (np.roll(text[:-1], 1) == ord("N")))[0]
    assert len(nruns) > 20
    r0 = int(nruns[0]) - 1  # the first letter of an N run
    qs = []
    for j in joins[:3]:
        q = bytes(text[j - 30:j + 31])
        qs += [q, q.replace(b"N", b"A"), q.replace(b"N", b"")]  # N in the read; a letter there: one edit; the join left out: one edit
    for a, b in ((r0 - 40, r0 + 3), (r0 - 40, r0 + 12), (r0 - 20, r0 + 1)):
        q = bytes(text[a:b])
        qs += [q, q.replace(b"N", b"C")]
    off, g, _, d, _ = check(nt, qs, k)
    assert d[off[0]:off[1]].min() == 0 and d[off[1]:off[2]].min() == 1 and d[off[2]:off[3]].min() == 1


@pytest.fixture(scope="module")
def aa():
    return World(*synth.make_text(5_000, 1, 53, 3, 0.01), 1)


@pytest.mark.parametrize("k", [1, 3])
def test_amino(aa, k):
    rng = np.random.default_rng(30 + k)
    qs = []
    for L in (12, 64, 65, 130):
        qs += reads_for(aa, rng, L, k)[0]
    off, g, _, d, _ = check(aa, qs, k)
    assert len(g) >= 12


@pytest.fixture(scope="module")
def family():
    """10 k random letters, then 3 000 copies of a 12-letter unit, each followed by 4 random letters"""
    rng = np.random.default_rng(54)
    rnd = lambda m: synth.NT[rng.integers(0, 4, size=m)]
    unit = np.frombuffer(b"GATTACAGGCTC", np.uint8)
    copies = np.concatenate([np.concatenate([unit, rnd(4)]) for _ in range(3000)])
    text = np.concatenate([rnd(10_000), copies, np.frombuffer(b"$", np.uint8)])
    return World(text, [0], ["r0"], 0)


def test_candidate_cap(family):
    w, rng = family, np.random.default_rng(55)
    qs = []
    for i in range(8):
        p = 10_000 + 16 * int(rng.integers(0, 2990))
        qs.append(bytes(w.text[p:p + 24]))                                  # piece 0 is the unit: 3 000 occurrences
        qs.append(planted(w, rng, 24, random_ops(rng, 24, i % 2))[0] if i % 2 else bytes(w.text[100 * i:100 * i + 24]))  # anywhere
    qs.append(bytes(w.text[500:524]))
    cands = [er.candidates(w.t.ctext, q, 1, 0) for q in qs]
    assert sum(c > 1000 for c in cands) >= 8 and sum(c <= 1000 for c in cands) >= 5
    off, g, _, d, st = check(w, qs, 1, max_candidates=1000)
    assert [int(s) for s in st] == [Q_CANDIDATE_CAP if c > 1000 else 0 for c in cands]  # exactly the reads the cap rule names
    for i, c in enumerate(cands):
        assert (off[i + 1] == off[i]) if c > 1000 else (off[i + 1] > off[i])   # abandoned: no hits; their neighbours: untouched
    check(w, qs, 1, max_candidates=10 ** 6)
    c0 = cands[-1]  # c(q) == max_candidates is not over the cap
    assert w.ix.parallel_locate_edit_csr(*pack_queries(qs[-1:]), 1, c0)[4][0] == 0
    if c0 > 1:
        assert w.ix.parallel_locate_edit_csr(*pack_queries(qs[-1:]), 1, c0 - 1)[4][0] == Q_CANDIDATE_CAP


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def test_results_do_not_depend_on_accelerators_chunks_or_replicas(nt):
    rng = np.random.default_rng(60)
    qs = []
    for L in (20, 64, 101, 129):
        qs += reads_for(nt, rng, L, 2)[0]
    qb, qo = pack_queries(qs)
    ix = nt.ix
    run = lambda x=ix: x.parallel_locate_edit_csr(qb, qo, 2, NO_CAP)
    base = check(nt, qs, 2)
    assert ix.verify_enabled()
    ix.set_verify(-1)  # the scan reads its own copy of the text, and leaves the knob alone
    try:
        assert not ix.verify_enabled()
        assert same(run(), base)
        assert not ix.verify_enabled()
    finally:
        ix.set_verify(2)
    assert ix.verify_enabled() and same(run(), base)
    ix.set_lcx(False)
    try:
        assert same(run(), base)
    finally:
        ix.set_lcx(True)
    ix.set_seed_kmer_len(0)
    try:
        assert ix.seed_kmer_len() == 0 and same(run(), base)
    finally:
        ix.set_seed_kmer_len(-1)
    assert sum(er.candidates(nt.t.ctext, q, 2, 0) for q in qs) > 40
    os.environ["AWRY_EDIT_CANDIDATE_CAP"] = "20"  # the chunk splits in halves, down to single queries
    try:
        assert same(run(), base)
    finally:
        del os.environ["AWRY_EDIT_CANDIDATE_CAP"]
    two = FmIndex.from_text(nt.text, 0, 8, 0, [int(s) for s in nt.st], ["seq%d" % i for i in range(len(nt.st))]).set_devices([0, 0])
    try:
        assert same(run(two), base)
    finally:
        two.close()


def test_rejected_queries_and_wide_rows(nt):
    ix = nt.ix
    good = bytes(nt.text[100:140])
    for bad, k in ((b"A" * 257, 1), (b"ACG", 3), (b"AC", 5), (b"", 0), (b"ACGT$ACGT", 1), (bytes([65, 200, 67, 71]), 1)):
        with pytest.raises(AwryError) as e:
            ix.parallel_locate_edit_csr(*pack_queries([good, bad, good]), k, NO_CAP)
        assert e.value.code == ERR_INVALID_QUERY, bad
    assert ix.count_string_edit(good, 1, NO_CAP) >= 1
    assert ix.locate_string_edit(b"ACGTACGTAC" * 25 + b"ACGTAC", 8, NO_CAP) is not None  # 256 letters, k = 8: the limits themselves
    L_ = awry_amd.load_library()
    L_.awry_debug_force_wide_rows(1)
    try:
        wide = FmIndex.from_text(nt.text[:3000].tobytes() + b"$", 0, 8, 0, [0], ["r"]).set_devices([0])
    finally:
        L_.awry_debug_force_wide_rows(0)
    try:
        with pytest.raises(AwryError) as e:
            wide.parallel_locate_edit_csr(*pack_queries([good]), 1, NO_CAP)
        assert e.value.code == ERR_ARG
    finally:
        wide.close()


def dev_windows(w, qs, wins, k, tally=False):
    """dev_edit_windows on hand-made windows [(query, first, count)] -> (n_hits[m], gpos, edits, tally or None)"""
    ix = w.ix
    qb, qo = pack_queries(qs)
    m = len(wins)
    pad = np.concatenate([qb, np.zeros(16, np.uint8)])
    ptrs = [ix.dev_upload(a) for a in (pad, qo, np.array([x[0] for x in wins], np.uint32), np.array([x[1] for x in wins], np.uint64),
                                       np.array([x[2] for x in wins], np.uint32))]
    d_n, d_off, d_scr, d_t = ix.dev_malloc(8 * m), ix.dev_malloc(8 * (m + 1)), ix.dev_malloc(ix.dev_scan_scratch_bytes(m)), ix.dev_malloc(16)
    ix.dev_memset(d_t, 0, 16)
    if tally:
        ix.dev_edit_windows_tally(*ptrs, m, k, d_n, d_t)
    else:
        ix.dev_edit_windows(*ptrs, m, k, d_n)
    ix.dev_scan_counts(d_n, m, d_off, d_scr)
    ix.dev_synchronize()
    n_hits = ix.dev_download(d_n, (m,), np.uint64)
    off = ix.dev_download(d_off, (m + 1,), np.uint64)
    tot = int(off[-1])
    assert tot == int(n_hits.sum())
    d_g, d_e = ix.dev_malloc(8 * max(tot, 1)), ix.dev_malloc(max(tot, 1))
    ix.dev_edit_windows(*ptrs, m, k, None, d_off, d_g, d_e)
    ix.dev_synchronize()
    g = ix.dev_download(d_g, (tot,), np.uint64) if tot else np.zeros(0, np.uint64)
    e = ix.dev_download(d_e, (tot,), np.uint8) if tot else np.zeros(0, np.uint8)
    t = ix.dev_download(d_t, (2,), np.uint64) if tally else None
    for p in ptrs + [d_n, d_off, d_scr, d_t, d_g, d_e]:
        ix.dev_free(p)
    return n_hits, g, e, t


def test_device_primitive_on_hand_made_windows(nt):
    rng = np.random.default_rng(70)
    k = 2
    q0, p0 = planted(nt, rng, 101, [("s", 30), ("d", 70)], p=5000)
    q1 = bytes(nt.text[:40])
    q2, _ = planted(nt, rng, 200, [("i", 100)], p=12_000)
    qs = [q0, q1, q2, b"A" * 12]
    n = nt.n
    wins = [(0, 5000, 1), (0, 4999, 1),                                  # single starts
            (1, 0, n), (3, 0, n),                                        # the whole text as one window
            (2, 11_900, 50), (2, 11_950, 60), (2, 12_010, 1), (2, 12_011, 200),   # adjacent windows that tile a region
            (1, 0, 1), (0, n - 1, 5), (0, n + 7, 3), (0, 100, 0)]        # start 0; cut at n; beyond n and empty: nothing
    n_hits, g, e, t = dev_windows(nt, qs, wins, k, tally=True)
    want_g, want_e, cols, scanned = [], [], 0, 0
    for (qi, first, count), got in zip(wins, n_hits):
        p, d = er.hits_of(nt.t.D(qs[qi]), k, first, first + count)
        assert int(got) == len(p), (qi, first, count)
        want_g.append(p.astype(np.uint64))
        want_e.append(d)
        cnt = min(first + count, n) - first
        if cnt > 0:
            a, b = er.scanned(first, cnt, len(qs[qi]), k, n)
            cols += b - a
            scanned += 1
    assert np.array_equal(g, np.concatenate(want_g)) and np.array_equal(e, np.concatenate(want_e))
    assert n_hits[0] == 1 and n_hits[2] >= 1 and n_hits[4:8].sum() >= 1
    assert [int(v) for v in t] == [cols, scanned]
    again = dev_windows(nt, qs, wins, k)
    assert np.array_equal(again[0], n_hits) and np.array_equal(again[1], g) and np.array_equal(again[2], e)


def test_seven_reads_halved_down_to_single_reads_equal_the_uncapped_call(nt):
    qs = reads_for(nt, np.random.default_rng(61), 101, 2)[0][:7]
    qb, qo = pack_queries(qs)
    want = nt.ix.parallel_align_edit_csr(qb, qo, 2, NO_CAP)
    assert len(qs) == 7 and int(want[0][-1]) >= 4
    os.environ["AWRY_EDIT_CANDIDATE_CAP"] = "1"  # every chunk of more than one read is over capacity
    try:
        got = nt.ix.parallel_align_edit_csr(qb, qo, 2, NO_CAP)
    finally:
        del os.environ["AWRY_EDIT_CANDIDATE_CAP"]
    assert len(got) == len(want) and same(got, want)
