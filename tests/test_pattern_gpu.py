"""Class-pattern count and locate on the GPU (the class mode of awry_amd/csrc/mismatch_kernels.hip.h) against tests/pattern_ref.py: the
brute-force definition (counts, positions, distances), the oracle's locate lists of the matched strings (order), the existing
exact and mismatch paths (plain-letter patterns, bit for bit), the stack bound (a planted text that fills all 18 frames), the
expansion cap, and independence of accelerators, SA ratio, replicas, row width, leaf capacity, lane refill and streams."""
import os
import threading
import time

import numpy as np
import pytest

from awry_amd.fm_index import ERR_INVALID_QUERY, AwryError, FmIndex, LocalizedSequencePosition, pack_queries
from tests import mismatch_ref as mr
from tests import pattern_ref as pr
from tests import synth
from tests import test_mismatch_gpu as tmg

pytestmark = pytest.mark.gpu

Q_EMPTY, Q_SENTINEL, Q_NON_ASCII, Q_NOT_CLASS_LETTER, Q_CLASS_POSITIONS, Q_EXPANSION_CAP = 1, 2, 3, 4, 5, 6
LENGTHS = (1, 2, 3, 5, 8, 12, 17, 25, 31, 64, 101)
CLASS_COUNTS = (0, 1, 2, 4, 8, 16)
LANES_PER_CU = 2048  # 8 waves x 4 SIMDs x 64 lanes: the ceiling on resident lanes per CU whatever the kernel's registers


def check_against_brute_force(ix, text, patterns, alphabet, ks=(0, 1, 2)):
    tsym = mr.to_symbols(text, alphabet)
    qb, qo = pack_queries(patterns)
    dists = [pr.window_dist(tsym, bytes(q), alphabet) for q in patterns]
    for k in ks:
        t0 = time.time()
        counts = ix.parallel_count_pattern_csr(qb, qo, k)
        off, gpos, pos, mm = ix.parallel_locate_pattern_csr(qb, qo, k)
        print("pattern coverage (alphabet %d, k = %d): %d patterns, %d hits, count + locate %.2f s" % (alphabet, k, len(patterns), int(off[-1]), time.time() - t0))
        assert counts.shape == (len(patterns), k + 1)
        assert np.array_equal(np.diff(off.astype(np.int64)), counts.sum(axis=1).astype(np.int64)), k
        for i, (q, dist) in enumerate(zip(patterns, dists)):
            ok = (dist >= 0) & (dist <= k)
            want = np.bincount(dist[ok], minlength=k + 1)[:k + 1]
            assert np.array_equal(counts[i], want), (bytes(q), k, counts[i], want)
            g = gpos[off[i]:off[i + 1]].astype(np.int64)
            d = mm[off[i]:off[i + 1]]
            order = np.argsort(g, kind="stable")
            wp = np.nonzero(ok)[0]
            assert np.array_equal(g[order], wp), (bytes(q), k)
            assert np.array_equal(d[order], dist[wp].astype(np.uint8)), (bytes(q), k)
            if len(g):  # one spot check per pattern: localisation itself is the exact path's, tested elsewhere
                rec, loc = pos[off[i]]
                assert ix.get_seq_location(int(g[0])) == LocalizedSequencePosition(int(rec), int(loc))
    return counts


def class_window(text, L, c, seed, alphabet, rng):
    """a window of the text and the c positions of it that get a class letter.  Amino patterns with 8 or 16 class positions: X
    holds every residue, so a suffix of X's -- and at k = 2 of X's and up to two plain letters -- walks the whole suffix trie
    of the 60 000 residues, level by level: six such levels are 200 000 expansions in one lane (a second of amino expansions),
    sixteen are the expansion cap itself.  Those patterns take the window richest in residues that a two-residue class holds
    (D N E Q I L) out of 200 drawn, put their class positions there first, and draw the narrowest class that holds; X fills
    the rest.  (Runs of X stay covered by the patterns with 4 class positions, by CxxC, HxxxH and by the full-stack test.)"""
    if alphabet == 0 or c < 8:
        return bytes(synth.sampled_queries(text, 1, L, seed, alphabet=alphabet)[0]), rng.choice(L, c, replace=False)
    cand = synth.sampled_queries(text, 200, L, seed, alphabet=1)
    two = np.isin(cand, np.frombuffer(b"DNEQIL", np.uint8))
    w = cand[int(np.argmax(two.sum(axis=1)))]
    order = np.lexsort((rng.random(L), ~np.isin(w, np.frombuffer(b"DNEQIL", np.uint8))))
    return bytes(w), order[:c]


def coverage_patterns(text, st, alphabet, seed):
    """windows of every length of LENGTHS with 0, 1, 2, 4, 8, 16 positions replaced by a class letter -- once with classes that
    all hold the text's letter, once with classes that all do not, once with one or two that do not -- the fixed patterns,
    windows across record joins and runs of the ambiguity symbol, lower case and U"""
    rng = np.random.default_rng(seed)
    pats, zero_at_k0 = [], []
    for L in LENGTHS:
        for c in CLASS_COUNTS:
            if c > L:
                continue
            w, positions = class_window(text, L, c, seed + 7 * L + c, alphabet, rng)
            narrow = alphabet == 1 and c >= 8
            pats.append(pr.replace_with_classes(w, positions, np.ones(c, bool), alphabet, rng, narrow))
            if c:
                pats.append(pr.replace_with_classes(w, positions, np.zeros(c, bool), alphabet, rng))
                hold = np.ones(c, bool)
                hold[rng.choice(c, min(c, int(rng.integers(1, 3))), replace=False)] = False
                pats.append(pr.replace_with_classes(w, positions, hold, alphabet, rng, narrow))
    amb = ord("N") if alphabet == 0 else ord("X")
    for s in st[1:3]:  # across record joins: the joining symbol is in no class
        zero_at_k0.append(bytes(text[s - 6:s + 9]))
    run = np.flatnonzero((text[:-1] == amb) & (np.roll(text[:-1], 1) == amb) & (np.roll(text[:-1], -1) == amb))
    first = int(run[0]) - 1  # first symbol of a run of the ambiguity symbol
    zero_at_k0.append(bytes(text[first - 12:first + 1]))
    zero_at_k0.append(bytes(text[first - 9:first + 2]))
    z0 = len(pats)
    pats += zero_at_k0
    if alphabet == 0:
        p = int(rng.integers(0, len(text) - 40))
        w = bytes(synth.sampled_queries(text, 1, 23, seed + 1)[0])
        pats += [b"RYRYRYRY", b"GANTC", w[:20] + b"NGG", bytes(text[p:p + 30]).lower().replace(b"n", b"a"),
                 bytes(text[p:p + 30]).replace(b"T", b"U").replace(b"N", b"A"), b"ganuc", b"ryRYswKMbdHVn"]
    else:
        w = bytes(synth.sampled_queries(text, 1, 21, seed + 1, alphabet=1)[0])
        pats += [b"C" + w[1:3].lower() + b"C", b"CxxC", b"bzjX", w[:1] + b"XXX" + w[4:5], w.lower()]
    return pats, slice(z0, z0 + len(zero_at_k0))


@pytest.fixture(scope="module")
def nt_text():
    return synth.make_text(40_000, 0, 21, 5, 0.03)


@pytest.fixture(scope="module")
def nt_index(nt_text):
    text, st, hd = nt_text
    return FmIndex.from_text(text, 0, 8, 0, st, hd).set_devices([0])


@pytest.fixture(scope="module")
def aa_text():
    return synth.make_text(60_000, 1, 22, 5, 0.01)


@pytest.fixture(scope="module")
def aa_index(aa_text):
    text, st, hd = aa_text
    return FmIndex.from_text(text, 1, 8, 0, st, hd).set_devices([0])


@pytest.mark.parametrize("k", [0, 1, 2])
def test_nucleotide_coverage_against_brute_force(nt_index, nt_text, k):
    text, st, _ = nt_text
    pats, zero = coverage_patterns(text, st, 0, 5)
    counts = check_against_brute_force(nt_index, text, pats, 0, (k,))
    z = counts[zero]
    assert (z[:, 0] == 0).all()       # a window over a join or a text N: nothing at k = 0 ...
    if k == 2:
        assert (z.sum(axis=1) >= 1).all()  # ... and itself, at one mismatch per such symbol (each holds at most two)


@pytest.mark.parametrize("k", [0, 1, 2])
def test_amino_coverage_against_brute_force(aa_index, aa_text, k):
    text, st, _ = aa_text
    pats, zero = coverage_patterns(text, st, 1, 6)
    counts = check_against_brute_force(aa_index, text, pats, 1, (k,))
    z = counts[zero]
    assert (z[:, 0] == 0).all()
    if k == 2:
        assert (z.sum(axis=1) >= 1).all()


def _status_of(ix, patterns, k=1):
    qb, qo = pack_queries(patterns)
    n = len(patterns)
    d_q, d_o = ix.dev_upload(np.concatenate([qb, np.zeros(16, np.uint8)])), ix.dev_upload(qo)
    d_c, d_s = ix.dev_malloc(8 * n * (k + 1)), ix.dev_malloc(n + 8)
    try:
        ix.dev_memset(d_c, 0x5A, 8 * n * (k + 1))
        ix.dev_memset(d_s, 0x5A, n)
        ix.dev_count_pattern(d_q, d_o, n, k, d_c, d_s)
        ix.dev_synchronize()
        return ix.dev_download(d_s, (n,), np.uint8), ix.dev_download(d_c, (n, k + 1), np.uint64)
    finally:
        for p in (d_q, d_o, d_c, d_s):
            ix.dev_free(p)


def test_rejected_patterns(nt_index, aa_index):
    cases = {0: [(b"N" * 17, Q_CLASS_POSITIONS, "class positions"), (b"ACGT" + b"RYSWKMBDHVNNNNNNN" + b"ACGT", Q_CLASS_POSITIONS, "class positions"),
                 (b"ACXG", Q_NOT_CLASS_LETTER, "class letter"), (b"AC-G", Q_NOT_CLASS_LETTER, "class letter"), (b"", Q_EMPTY, "empty"),
                 (b"AC$T", Q_SENTINEL, "'$'"), (b"A#", Q_SENTINEL, "'$'"), (bytes([0x41, 0x80]), Q_NON_ASCII, "non-ASCII")],
             1: [(b"X" * 17, Q_CLASS_POSITIONS, "class positions"), (b"MKUV", Q_NOT_CLASS_LETTER, "class letter"),
                 (b"MK*", Q_NOT_CLASS_LETTER, "class letter"), (b"M-K", Q_NOT_CLASS_LETTER, "class letter"), (b"", Q_EMPTY, "empty"),
                 (b"MK$", Q_SENTINEL, "'$'"), (bytes([0x4D, 0xC3, 0xA9]), Q_NON_ASCII, "non-ASCII")]}
    for alphabet, ix in ((0, nt_index), (1, aa_index)):
        good = [b"ACGT", b"GGA"] if alphabet == 0 else [b"MKV", b"LLA"]
        ok_counts = ix.parallel_count_pattern(good, 1)
        for bad, status, word in cases[alphabet]:
            qb, qo = pack_queries([good[0], bad, good[1]])
            for call in (ix.parallel_count_pattern_csr, ix.parallel_locate_pattern_csr):
                with pytest.raises(AwryError) as e:
                    call(qb, qo, 1)
                assert e.value.code == ERR_INVALID_QUERY, bad
                assert "query 1:" in str(e.value) and word in str(e.value), (bad, str(e.value))
            st, counts = _status_of(ix, [good[0], bad, good[1]])
            assert list(st) == [0, status, 0], (bad, st)
            assert not counts[1].any() and np.array_equal(counts[[0, 2]], ok_counts), bad
        # exactly 16 class positions are accepted
        edge = b"N" * 16 + b"ACGTAC" if alphabet == 0 else b"X" * 16 + b"L"
        assert list(_status_of(ix, [edge], 0)[0]) == [0]


def plain_letter_queries(text, st):
    qs = tmg.coverage_queries(text, st, seed=9) + [bytes(q) for q in synth.sampled_queries(text, 500, 31, 4)]
    qs = [bytes(b for b in q if b in b"ACGTUacgtu") for q in qs]
    return [q for q in qs if q]


def test_plain_letter_patterns_equal_the_mismatch_and_exact_paths(nt_index, nt_text):
    text, st, _ = nt_text
    qs = plain_letter_queries(text, st)
    assert len(qs) > 550
    qb, qo = pack_queries(qs)
    for k in (0, 1, 2):
        assert np.array_equal(nt_index.parallel_count_pattern_csr(qb, qo, k), nt_index.parallel_count_mismatch_csr(qb, qo, k)), k
        got, want = nt_index.parallel_locate_pattern_csr(qb, qo, k), nt_index.parallel_locate_mismatch_csr(qb, qo, k)
        assert all(x.shape == y.shape and np.array_equal(x, y) for x, y in zip(got, want)), k
    c0 = nt_index.parallel_count_pattern_csr(qb, qo, 0)
    assert np.array_equal(c0[:, 0], nt_index.parallel_count_csr(qb, qo))
    off, gpos, pos, mm = nt_index.parallel_locate_pattern_csr(qb, qo, 0)
    eoff, egpos, epos = nt_index.parallel_locate_csr(qb, qo)
    assert np.array_equal(off, eoff) and np.array_equal(gpos, egpos) and np.array_equal(pos, epos) and not mm.any()


def test_plain_letter_patterns_equal_the_mismatch_path_amino(aa_index, aa_text):
    text, st, _ = aa_text
    qs = [bytes(q) for L in (1, 2, 3, 5, 8, 12, 25) for q in synth.sampled_queries(text, 8, L, 60 + L, alphabet=1)]
    qs += [bytes(q) for q in synth.random_queries(20, 4, 1, 61)] + [b"mkvl", b"W"]
    qb, qo = pack_queries(qs)
    for k in (0, 1, 2):
        assert np.array_equal(aa_index.parallel_count_pattern_csr(qb, qo, k), aa_index.parallel_count_mismatch_csr(qb, qo, k)), k
        got, want = aa_index.parallel_locate_pattern_csr(qb, qo, k), aa_index.parallel_locate_mismatch_csr(qb, qo, k)
        assert all(x.shape == y.shape and np.array_equal(x, y) for x, y in zip(got, want)), k
    assert np.array_equal(aa_index.parallel_count_pattern_csr(qb, qo, 0)[:, 0], aa_index.parallel_count_csr(qb, qo))


@pytest.mark.parametrize("alphabet,n,lengths", [(0, 200_000, (6, 11, 16)), (1, 60_000, (3, 5, 7))], ids=["nucleotide", "amino"])
def test_locate_order_against_oracle_lists_of_the_matched_strings(oracle, alphabet, n, lengths):
    text, st, hd = synth.make_text(n, alphabet, 8, 3, 0.01)
    ix = FmIndex.from_text(text, alphabet, 8, 0, st, hd).set_devices([0])
    oi = oracle.OracleIndex.from_text(text, alphabet, 8, 0, st, hd)
    rng = np.random.default_rng(17 + alphabet)
    pats = []
    for i, L in enumerate(lengths):
        for c in (1, 2, 3, 4):
            if c > L:
                continue
            w = bytes(synth.sampled_queries(text, 1, L, 70 + 5 * L + c, alphabet=alphabet)[0])
            hold = np.ones(c, bool)
            hold[:(c + i) % 2] = False
            pats.append(pr.replace_with_classes(w, rng.choice(L, c, replace=False), hold, alphabet, rng))
    assert len(pats) >= 11
    qb, qo = pack_queries(pats)
    for k in (0, 1, 2):
        off, gpos, pos, mm = ix.parallel_locate_pattern_csr(qb, qo, k)
        counts = ix.parallel_count_pattern_csr(qb, qo, k)
        for i, p in enumerate(pats):
            g, pp, d = pr.ordered_hits(oi, text, p, k, alphabet)
            assert np.array_equal(gpos[off[i]:off[i + 1]], g), (alphabet, p, k)
            assert np.array_equal(pos[off[i]:off[i + 1]], pp), (alphabet, p, k)
            assert np.array_equal(mm[off[i]:off[i + 1]], d), (alphabet, p, k)
            assert np.array_equal(counts[i], pr.brute_force(text, p, k, alphabet)[0]), (alphabet, p, k)
    ix.close()


def _count_with_tally(ix, patterns, k):
    """-> (counts [n, k + 1], status [n], tally [3]) of one device call"""
    qb, qo = pack_queries(patterns)
    n = len(patterns)
    d_q, d_o = ix.dev_upload(np.concatenate([qb, np.zeros(16, np.uint8)])), ix.dev_upload(qo)
    d_c, d_s, d_t = ix.dev_malloc(8 * n * (k + 1)), ix.dev_malloc(n + 8), ix.dev_malloc(24)
    try:
        ix.dev_memset(d_t, 0, 24)
        ix.dev_count_pattern_tally(d_q, d_o, n, k, d_c, d_t, d_s)
        ix.dev_synchronize()
        return ix.dev_download(d_c, (n, k + 1), np.uint64), ix.dev_download(d_s, (n,), np.uint8), ix.dev_download(d_t, (3,), np.uint64)
    finally:
        for p in (d_q, d_o, d_c, d_s, d_t):
            ix.dev_free(p)


def full_stack_text():
    """4 000 random nucleotides with G + w + T planted for w = A x 18 and the sixteen A^j C A^(17 - j), j = 0 .. 15"""
    rng = np.random.default_rng(3)
    body = synth.NT[rng.integers(0, 4, size=4_000)].copy()
    plants = [b"G" + b"A" * 18 + b"T"] + [b"G" + b"A" * j + b"C" + b"A" * (17 - j) + b"T" for j in range(16)]
    for i, p in enumerate(plants):
        body[100 + 200 * i:100 + 200 * i + len(p)] = np.frombuffer(p, np.uint8)
    return np.concatenate([body, np.frombuffer(b"$", np.uint8)])


@pytest.mark.parametrize("alphabet", [0, 1], ids=["nucleotide", "amino"])
def test_full_stack_of_18_frames(alphabet):
    """G + 16 x (N or X) + GT at k = 2 on a text where, with the mismatching children visited first in ascending symbol index
    (the kernel's documented order), the path T->A, G->A, then sixteen A's holds a frame at every one of the 18 non-leaf levels:
    the frames beyond the two in registers go through the workspace and come back."""
    text = full_stack_text()
    ix = FmIndex.from_text(text, alphabet, 8, 0, [0], ["planted"]).set_devices([0])
    pat = b"G" + (b"N" if alphabet == 0 else b"X") * 16 + b"GT"
    want, pos, dist = pr.brute_force(text, pat, 2, alphabet)
    assert int(want.sum()) > 1000
    counts, status, tally = _count_with_tally(ix, [pat], 2)
    print("full stack (alphabet %d): %d expansions, deepest stack %d, %d hits" % (alphabet, int(tally[0]), int(tally[2]), int(want.sum())))
    assert list(status) == [0] and np.array_equal(counts[0], want)
    assert int(tally[1]) == 1 and int(tally[2]) == 18
    off, gpos, _, mm = ix.parallel_locate_pattern_csr(*pack_queries([pat]), 2, want_pos=False)
    order = np.argsort(gpos.astype(np.int64), kind="stable")
    assert np.array_equal(gpos.astype(np.int64)[order], pos) and np.array_equal(mm[order], dist)
    ix.close()


def test_expansion_cap(nt_index, nt_text, monkeypatch):
    text, st, _ = nt_text
    cheap = [bytes(q) for q in synth.sampled_queries(text, 6, 31, 80)] + [b"GANTC", b"ACGTTGCAAC"]
    pats = cheap[:4] + [b"N" * 12] + cheap[4:]
    want, status, tally = _count_with_tally(nt_index, pats, 0)
    assert not status.any() and int(tally[0]) > 64
    need = [int(_count_with_tally(nt_index, [p], 0)[2][0]) for p in cheap]
    assert max(need) <= 64 and int(_count_with_tally(nt_index, [b"N" * 12], 0)[2][0]) > 64
    monkeypatch.setenv("AWRY_PATTERN_MAX_EXPANSIONS", "64")
    qb, qo = pack_queries(pats)
    for call in (nt_index.parallel_count_pattern_csr, nt_index.parallel_locate_pattern_csr):
        with pytest.raises(AwryError) as e:
            call(qb, qo, 0)
        assert e.value.code == ERR_INVALID_QUERY and "query 4:" in str(e.value) and "expansion cap" in str(e.value), str(e.value)
    got, status, _ = _count_with_tally(nt_index, pats, 0)
    assert list(status) == [0, 0, 0, 0, Q_EXPANSION_CAP, 0, 0, 0, 0]
    assert not got[4].any() and np.array_equal(np.delete(got, 4, axis=0), np.delete(want, 4, axis=0))
    # a search that needs exactly the cap passes; one expansion less and it is abandoned
    exact = max(need)
    p = cheap[need.index(exact)]
    full = _count_with_tally(nt_index, [p], 0)[0]
    monkeypatch.setenv("AWRY_PATTERN_MAX_EXPANSIONS", str(exact))
    got, status, tally = _count_with_tally(nt_index, [p], 0)
    assert list(status) == [0] and np.array_equal(got, full) and int(tally[0]) == exact
    monkeypatch.setenv("AWRY_PATTERN_MAX_EXPANSIONS", str(exact - 1))
    got, status, _ = _count_with_tally(nt_index, [p], 0)
    assert list(status) == [Q_EXPANSION_CAP] and not got.any()


def _results(ix, qb, qo, k):
    return (ix.parallel_count_pattern_csr(qb, qo, k),) + tuple(ix.parallel_locate_pattern_csr(qb, qo, k))


def _same(a, b):
    return all(x.shape == y.shape and np.array_equal(x, y) for x, y in zip(a, b))


def test_results_do_not_depend_on_accelerators_ratio_replicas_row_width_or_capacity():
    import awry_amd
    text, st, hd = synth.make_text(100_000, 0, 12, 4, 0.02)
    rng = np.random.default_rng(4)
    pats = []
    for i, w in enumerate(synth.sampled_queries(text, 120, 20, 3)):
        c = i % 5
        hold = rng.random(c) < 0.8
        pats.append(pr.replace_with_classes(bytes(w), rng.choice(20, c, replace=False), hold, 0, rng))
    pats += [bytes(q) for q in synth.random_queries(30, 12, 0, 5)] + [b"GANTC", b"ryryryry", b"ACGUN"]
    qb, qo = pack_queries(pats)
    ix = FmIndex.from_text(text, 0, 8, 0, st, hd).set_devices([0])
    base = {k: _results(ix, qb, qo, k) for k in (0, 1, 2)}
    assert int(base[2][1][-1]) > 1000
    for knob in (lambda: ix.set_seed_kmer_len(0), lambda: ix.set_seed_kmer_len(-1), lambda: ix.set_lcx(False), lambda: ix.set_verify(-1),
                 lambda: ix.set_locate_sa_ratio(1), lambda: ix.set_locate_sa_ratio(0)):
        knob()
        for k in (0, 2):
            assert _same(_results(ix, qb, qo, k), base[k]), k
    os.environ["AWRY_MISMATCH_LEAF_CAP"] = "7"  # the capacity fallback: chunks split until each fits (or holds one pattern)
    try:
        for k in (1, 2):
            assert _same(_results(ix, qb, qo, k), base[k]), k
    finally:
        del os.environ["AWRY_MISMATCH_LEAF_CAP"]
    ix.set_devices([0, 0])
    for k in (0, 2):
        assert _same(_results(ix, qb, qo, k), base[k]), k
    ix.close()
    L = awry_amd.load_library()
    L.awry_debug_force_wide_rows(1)
    try:
        wx = FmIndex.from_text(text, 0, 8, 0, st, hd).set_devices([0])
    finally:
        L.awry_debug_force_wide_rows(0)
    for k in (0, 2):
        assert _same(_results(wx, qb, qo, k), base[k]), k
    wx.close()


# ---------------------------------------------------------------------------------------------- lane refill and streams

@pytest.fixture(scope="module")
def pool(nt_index, nt_text):
    """~300 patterns on the 40 kbp text with their brute-force counts at k = 2"""
    text, st, _ = nt_text
    rng = np.random.default_rng(41)
    pats = []
    for i in range(300):
        L = int(rng.integers(10, 32))
        w = bytes(synth.sampled_queries(text, 1, L, 500 + i)[0]) if i % 4 else bytes(synth.random_queries(1, L, 0, 500 + i)[0])
        c = (0, 0, 1, 2, 3, 4)[i % 6]
        pats.append(pr.replace_with_classes(w, rng.choice(L, c, replace=False), rng.random(c) < 0.8, 0, rng))
    counts = np.stack([pr.brute_force(text, p, 2, 0)[0] for p in pats])
    return pats, counts


def _draw_batch(pats, draw):
    """-> (bytes with 16 bytes of slack, offsets) of the patterns pats[draw]"""
    lens = np.array([len(p) for p in pats], np.int64)
    padded = np.zeros((len(pats), int(lens.max())), np.uint8)
    for i, p in enumerate(pats):
        padded[i, :len(p)] = np.frombuffer(p, np.uint8)
    used = np.arange(padded.shape[1])[None, :] < lens[:, None]
    qo = np.zeros(len(draw) + 1, np.uint64)
    qo[1:] = np.cumsum(lens[draw])
    return np.concatenate([padded[draw][used[draw]], np.zeros(16, np.uint8)]), qo


def test_lane_refill(nt_index, pool):
    import torch
    pats, counts = pool
    lanes = torch.cuda.get_device_properties(0).multi_processor_count * LANES_PER_CU
    n = 2 * lanes
    draw = np.random.default_rng(42).integers(0, len(pats), size=n)
    assert n >= 2 * lanes  # no launch has more lanes than `lanes`: every lane takes two patterns or more on average
    qb, qo = _draw_batch(pats, draw)
    d_q, d_o = torch.from_numpy(qb).cuda(), torch.from_numpy(qo.view(np.int64)).cuda()
    d_c = torch.full((n * 3,), 0x5A5A5A5A, dtype=torch.int64, device="cuda")
    d_s = torch.full((n,), 0x5A, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    t0 = time.time()
    nt_index.dev_count_pattern(d_q.data_ptr(), d_o.data_ptr(), n, 2, d_c.data_ptr(), d_s.data_ptr())
    torch.cuda.synchronize()
    print("lane refill: n = %d = 2 x %d lanes, device call %.2f s" % (n, lanes, time.time() - t0))
    assert not d_s.cpu().numpy().any()
    assert np.array_equal(d_c.cpu().numpy().view(np.uint64).reshape(n, 3), counts[draw])


def test_four_streams_three_launches_each_from_two_threads(nt_index, pool):
    import torch
    pats, counts = pool
    n = 1 << 15
    streams = [torch.cuda.Stream() for _ in range(4)]
    jobs = []
    for si in range(4):
        for j in range(3):
            draw = np.random.default_rng(100 + 10 * si + j).integers(0, len(pats), size=n)
            qb, qo = _draw_batch(pats, draw)
            jobs.append((si, draw, torch.from_numpy(qb).cuda(), torch.from_numpy(qo.view(np.int64)).cuda(),
                         torch.full((n * 3,), 0x5A5A5A5A, dtype=torch.int64, device="cuda"), torch.full((n,), 0x5A, dtype=torch.uint8, device="cuda")))
    torch.cuda.synchronize()
    errors = []

    def drive(mine):
        try:
            torch.cuda.set_device(0)
            for si, _, d_q, d_o, d_c, d_s in [j for j in jobs if j[0] in mine]:
                nt_index.dev_count_pattern(d_q.data_ptr(), d_o.data_ptr(), n, 2, d_c.data_ptr(), d_s.data_ptr(), streams[si].cuda_stream)
        except BaseException as e:  # noqa: BLE001
            errors.append(repr(e))

    threads = [threading.Thread(target=drive, args=(m,)) for m in ((0, 1), (2, 3))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    torch.cuda.synchronize()
    assert not errors, errors
    for si, draw, _, _, d_c, d_s in jobs:
        assert not d_s.cpu().numpy().any(), si
        assert np.array_equal(d_c.cpu().numpy().view(np.uint64).reshape(n, 3), counts[draw]), si
