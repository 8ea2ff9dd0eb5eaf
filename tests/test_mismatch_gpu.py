"""Substitution-tolerant count and locate on the GPU (awry_amd/csrc/mismatch_kernels.hip.h) against the two references of
tests/mismatch_ref.py: the brute-force definition (counts, positions, distances) and the oracle's per-variant locate lists
(order).  k = 0 must equal the exact path bit for bit; results must not depend on the accelerators, the SA ratio, the
number of replicas or the leaf capacity of the locate chunks."""
import os

import numpy as np
import pytest

from awry_amd.fm_index import ERR_INVALID_QUERY, AwryError, FmIndex, LocalizedSequencePosition, pack_queries
from tests import mismatch_ref as mr
from tests import pattern_ref, synth

pytestmark = pytest.mark.gpu


def brute_dist(tsym, query, alphabet):
    """distance of every window (-1 where it holds '$')"""
    q = mr.to_symbols(query, alphabet)
    L, n = len(q), len(tsym)
    W = n - L + 1
    dist = np.zeros(W, np.int32)
    sent = np.zeros(W, bool)
    for j in range(L):
        w = tsym[j:j + W]
        dist += w != q[j]
        sent |= w == 0
    dist[sent] = -1
    return dist


def check_against_brute_force(ix, text, queries, alphabet, ks=(0, 1, 2)):
    tsym = mr.to_symbols(text, alphabet)
    qb, qo = pack_queries(queries)
    dists = [brute_dist(tsym, bytes(q), alphabet) for q in queries]
    for k in ks:
        counts = ix.parallel_count_mismatch_csr(qb, qo, k)
        off, gpos, pos, mm = ix.parallel_locate_mismatch_csr(qb, qo, k)
        assert counts.shape == (len(queries), k + 1)
        assert np.array_equal(np.diff(off.astype(np.int64)), counts.sum(axis=1).astype(np.int64)), k
        for i, (q, dist) in enumerate(zip(queries, dists)):
            ok = (dist >= 0) & (dist <= k)
            want = np.bincount(dist[ok], minlength=k + 1)[:k + 1]
            assert np.array_equal(counts[i], want), (bytes(q), k, counts[i], want)
            g = gpos[off[i]:off[i + 1]].astype(np.int64)
            d = mm[off[i]:off[i + 1]]
            order = np.argsort(g, kind="stable")
            wp = np.nonzero(ok)[0]
            assert np.array_equal(g[order], wp), (bytes(q), k)
            assert np.array_equal(d[order], dist[wp].astype(np.uint8)), (bytes(q), k)
            if len(g):  # one spot check per query: localisation itself is the exact path's, tested elsewhere
                rec, loc = pos[off[i]]
                assert ix.get_seq_location(int(g[0])) == LocalizedSequencePosition(int(rec), int(loc))


@pytest.fixture(scope="module")
def nt_text():
    return synth.make_text(40_000, 0, 21, 5, 0.03)


@pytest.fixture(scope="module")
def nt_index(nt_text):
    text, st, hd = nt_text
    return FmIndex.from_text(text, 0, 8, 0, st, hd).set_devices([0])


def coverage_queries(text, st, seed=5, n_random=40):
    """ragged random queries, sampled ones with planted substitutions, windows across N runs and record joins, lowercase,
    U and IUPAC bytes"""
    rng = np.random.default_rng(seed)
    qs = []
    for L in rng.integers(1, 121, size=n_random):
        qs.append(bytes(synth.NT[rng.integers(0, 4, size=int(L))]))
    n = len(text) - 1
    for L in (1, 2, 3, 5, 8, 12, 17, 25, 31, 40, 64, 101, 120):
        p = int(rng.integers(0, n - L))
        q = bytearray(text[p:p + L])
        for _ in range(int(rng.integers(0, 3))):
            j = int(rng.integers(0, L))
            q[j] = b"ACGT"[(b"ACGT".find(bytes([q[j]])) + 1) % 4] if q[j] in b"ACGT" else ord("A")
        qs.append(bytes(q))
    for s in st[1:]:  # across record joins
        qs.append(bytes(text[s - 6:s + 9]))
    nrun = np.nonzero(text[:-1] == ord("N"))[0]
    if len(nrun):
        p = int(nrun[len(nrun) // 2])
        qs.append(bytes(text[max(0, p - 10):p + 10]))
        qs.append(bytes(text[int(nrun[0]) - 8:int(nrun[0]) + 4]))
    p = int(rng.integers(0, n - 30))
    qs.append(bytes(text[p:p + 30]).lower())
    qs.append(bytes(text[p:p + 30]).replace(b"T", b"U"))
    qs.append(bytes(text[p:p + 30]).replace(b"A", b"R", 2))
    qs.append(b"ACGTRYKMSWBDHVN")
    qs.append(b"acgtnnnnacgt")
    return qs


def test_rank_all_equals_rank_of_every_symbol(oracle):
    for alphabet in (0, 1):
        text, st, hd = synth.make_text(5_000, alphabet, 3, 3, 0.02)
        ix = FmIndex.from_text(text, alphabet, 8, 0, st, hd).set_devices([0])
        oi = oracle.OracleIndex.from_text(text, alphabet, 8, 0, st, hd)
        n = ix.bwt_len()
        rows = np.unique(np.concatenate([np.arange(0, n, 37), [0, 1, 63, 64, 255, 256, 257, n - 2, n - 1]])).astype(np.uint64)
        got = ix.debug_rank_all(rows)
        S = got.shape[1]
        want = np.array([[oi.global_occurrence(int(r), s) for s in range(1, S + 1)] for r in rows], np.uint64)
        assert np.array_equal(got, want), alphabet


def test_nucleotide_input_coverage_against_brute_force(nt_index, nt_text):
    text, st, _ = nt_text
    check_against_brute_force(nt_index, text, coverage_queries(text, st), 0)


def test_k0_equals_the_exact_path_bit_for_bit(nt_index, nt_text):
    text, st, _ = nt_text
    qs = coverage_queries(text, st, seed=9) + [bytes(q) for q in synth.sampled_queries(text, 500, 31, 4)]
    qb, qo = pack_queries(qs)
    c0 = nt_index.parallel_count_mismatch_csr(qb, qo, 0)
    assert np.array_equal(c0[:, 0], nt_index.parallel_count_csr(qb, qo))
    off, gpos, pos, mm = nt_index.parallel_locate_mismatch_csr(qb, qo, 0)
    eoff, egpos, epos = nt_index.parallel_locate_csr(qb, qo)
    assert np.array_equal(off, eoff) and np.array_equal(gpos, egpos) and np.array_equal(pos, epos)
    assert not mm.any()


def test_locate_order_and_distances_against_oracle_variants(oracle):
    for alphabet, n, L, ks in ((0, 200_000, (6, 11, 16), (1, 2)), (1, 60_000, (3, 5, 7), (1, 2))):
        text, st, hd = synth.make_text(n, alphabet, 8, 3, 0.01)
        ix = FmIndex.from_text(text, alphabet, 8, 0, st, hd).set_devices([0])
        oi = oracle.OracleIndex.from_text(text, alphabet, 8, 0, st, hd)
        qs = [bytes(synth.sampled_queries(text, 1, l, 30 + l, alphabet=alphabet)[0]) for l in L]
        qs += [bytes(synth.random_queries(1, l, alphabet, 40 + l)[0]) for l in L]
        qb, qo = pack_queries(qs)
        for k in ks:
            off, gpos, pos, mm = ix.parallel_locate_mismatch_csr(qb, qo, k)
            counts = ix.parallel_count_mismatch_csr(qb, qo, k)
            for i, q in enumerate(qs):
                g, p, d = mr.oracle_locate(oi, q, k, alphabet)
                assert np.array_equal(gpos[off[i]:off[i + 1]], g), (alphabet, q, k)
                assert np.array_equal(pos[off[i]:off[i + 1]], p), (alphabet, q, k)
                assert np.array_equal(mm[off[i]:off[i + 1]], d), (alphabet, q, k)
                assert np.array_equal(counts[i], mr.oracle_counts(oi, q, k, alphabet)), (alphabet, q, k)


def test_repeat_rich_text_and_amino(oracle):
    text, st, hd, _ = synth.repeat_rich_text(400_000, seed=5, n_records=3, device="cpu", scale=2.0)
    ix = FmIndex.from_text(text, 0, 8, 0, st, hd).set_devices([0])
    qs = [bytes(q) for q in synth.sampled_queries(text, 24, 20, 6)] + [bytes(q) for q in synth.sampled_queries(text, 8, 12, 7)]
    check_against_brute_force(ix, text, qs, 0)
    atext, ast, ahd = synth.make_text(50_000, 1, 9, 4, 0.01)
    aix = FmIndex.from_text(atext, 1, 8, 0, ast, ahd).set_devices([0])
    aq = [bytes(q) for q in synth.sampled_queries(atext, 10, 8, 3, alphabet=1)] + [bytes(q) for q in synth.random_queries(6, 5, 1, 4)]
    aq += [b"mkvB", bytes(atext[ast[1] - 3:ast[1] + 4]), b"W"]
    check_against_brute_force(aix, atext, aq, 1, ks=(1, 2))


def _results(ix, qb, qo, k):
    return (ix.parallel_count_mismatch_csr(qb, qo, k),) + tuple(ix.parallel_locate_mismatch_csr(qb, qo, k))


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def test_results_do_not_depend_on_accelerators_ratio_replicas_or_capacity():
    text, st, hd = synth.make_text(300_000, 0, 12, 4, 0.02)
    qs = [bytes(q) for q in synth.sampled_queries(text, 300, 25, 3)] + [bytes(q) for q in synth.random_queries(100, 14, 0, 5)]
    qs += [b"ACGTN", b"acgtu" * 3]
    qb, qo = pack_queries(qs)
    for ratio in (1, 8):
        ix = FmIndex.from_text(text, 0, ratio, 0, st, hd).set_devices([0])
        base = {k: _results(ix, qb, qo, k) for k in (0, 1, 2)}
        for knob in (lambda: ix.set_seed_kmer_len(0), lambda: ix.set_verify(-1), lambda: ix.set_lcx(False), lambda: ix.set_lcx(True),
                     lambda: ix.set_locate_sa_ratio(1), lambda: ix.set_locate_sa_ratio(0), lambda: ix.set_seed_kmer_len(-1),
                     lambda: ix.set_verify(2)):
            knob()
            for k in (1, 2):
                assert _same(_results(ix, qb, qo, k), base[k]), k
        os.environ["AWRY_MISMATCH_LEAF_CAP"] = "7"  # the capacity fallback: chunks split until each fits (or holds one query)
        try:
            for k in (1, 2):
                assert _same(_results(ix, qb, qo, k), base[k]), k
        finally:
            del os.environ["AWRY_MISMATCH_LEAF_CAP"]
        ix.set_devices([0, 0])
        for k in (0, 2):
            assert _same(_results(ix, qb, qo, k), base[k]), k
        ix.close()


def test_ratio_1_and_8_agree():
    text, st, hd = synth.make_text(100_000, 0, 13, 2, 0.01)
    qs = [bytes(q) for q in synth.sampled_queries(text, 100, 18, 8)]
    qb, qo = pack_queries(qs)
    a = FmIndex.from_text(text, 0, 1, 0, st, hd).set_devices([0])
    b = FmIndex.from_text(text, 0, 8, 0, st, hd).set_devices([0])
    for k in (1, 2):
        assert _same(_results(a, qb, qo, k), _results(b, qb, qo, k))


def test_invalid_query_in_a_batch_is_rejected(nt_index):
    for bad in (b"AC$T", b"", b"A#", bytes([0x41, 0x80])):
        qb, qo = pack_queries([b"ACGT", bad, b"GGA"])
        for call in (nt_index.parallel_count_mismatch_csr, nt_index.parallel_locate_mismatch_csr):
            with pytest.raises(AwryError) as e:
                call(qb, qo, 1)
            assert e.value.code == ERR_INVALID_QUERY, bad


def test_device_resident_count_and_census(nt_index, nt_text):
    text, st, _ = nt_text
    qs = coverage_queries(text, st, seed=11)
    qb, qo = pack_queries(qs)
    n = len(qs)
    d_q, d_o = nt_index.dev_upload(np.concatenate([qb, np.zeros(16, np.uint8)])), nt_index.dev_upload(qo)
    d_c, d_t = nt_index.dev_malloc(8 * n * 3), nt_index.dev_malloc(16)
    try:
        nt_index.dev_memset(d_t, 0, 16)
        nt_index.dev_count_mismatch_tally(d_q, d_o, n, 2, d_c, d_t)
        nt_index.dev_synchronize()
        got = nt_index.dev_download(d_c, (n, 3), np.uint64)
        tally = nt_index.dev_download(d_t, (2,), np.uint64)
        nt_index.dev_count_mismatch(d_q, d_o, n, 2, d_c)
        nt_index.dev_synchronize()
        again = nt_index.dev_download(d_c, (n, 3), np.uint64)
    finally:
        for p in (d_q, d_o, d_c, d_t):
            nt_index.dev_free(p)
    want = nt_index.parallel_count_mismatch_csr(qb, qo, 2)
    assert np.array_equal(got, want) and np.array_equal(again, want)
    assert int(tally[1]) == n and int(tally[0]) >= n
    assert nt_index.count_string_mismatch(qs[-6], 2) == int(want[-6].sum())
    assert len(nt_index.locate_string_mismatch(qs[-6], 1)) == int(want[-6][:2].sum())


def _dev_count_with_tally(ix, qs, k):
    """-> (counts uint64[n, k + 1], status uint8[n], census uint64[2]) of one dev_count_mismatch_tally launch; the census buffer
    is the 16 bytes the letter mode may write"""
    qb, qo = pack_queries(qs)
    n = len(qs)
    d_q, d_o = ix.dev_upload(np.concatenate([qb, np.zeros(16, np.uint8)])), ix.dev_upload(qo)
    d_c, d_t, d_s = ix.dev_malloc(8 * n * (k + 1)), ix.dev_malloc(16), ix.dev_malloc(n)
    try:
        ix.dev_memset(d_t, 0, 16)
        ix.dev_count_mismatch_tally(d_q, d_o, n, k, d_c, d_t, d_s)
        ix.dev_synchronize()
        return ix.dev_download(d_c, (n, k + 1), np.uint64), ix.dev_download(d_s, (n,), np.uint8), ix.dev_download(d_t, (2,), np.uint64)
    finally:
        for p in (d_q, d_o, d_c, d_t, d_s):
            ix.dev_free(p)


def test_the_letter_path_has_no_expansion_cap(nt_index, nt_text, monkeypatch):
    """AWRY_PATTERN_MAX_EXPANSIONS is the class mode's: the letter mode of the same kernel must not see it"""
    text, _, _ = nt_text
    qs = [bytes(q) for q in synth.sampled_queries(text, 8, 31, 17)]
    qb, qo = pack_queries(qs)

    def run():
        return _results(nt_index, qb, qo, 2) + _dev_count_with_tally(nt_index, qs, 2)

    first = run()
    assert not first[-2].any() and int(first[-1][1]) == len(qs)
    for q in qs:  # a cap of 1 would fire on every query
        _, status, census = _dev_count_with_tally(nt_index, [q], 2)
        assert list(status) == [0] and int(census[1]) == 1 and int(census[0]) > 1, q
    monkeypatch.setenv("AWRY_PATTERN_MAX_EXPANSIONS", "1")
    assert _same(run(), first)
    with pytest.raises(AwryError) as e:  # the setting is live: the class mode abandons the same queries
        nt_index.parallel_count_pattern_csr(qb, qo, 2)
    assert e.value.code == ERR_INVALID_QUERY and "expansion cap" in str(e.value), str(e.value)


def test_letters_and_classes_stay_two_tables(nt_index, nt_text):
    """an IUPAC byte is the symbol N on the mismatch entry points and a class on the pattern entry points"""
    text, _, _ = nt_text
    n = len(text) - 1
    p = next(p for p in range(1000, n - 12) if b"N" not in bytes(text[p:p + 12]) and b"$" not in bytes(text[p:p + 12])
             and (b"A" in bytes(text[p:p + 12]) or b"G" in bytes(text[p:p + 12])))
    w = bytearray(text[p:p + 12])
    j = next(j for j in range(12) if w[j] in b"AG")
    w[j] = ord("R")
    qs = [bytes(w), b"ACGTRYKMSWBDHVN"]
    qb, qo = pack_queries(qs)
    paths = ((mr.brute_force, nt_index.parallel_count_mismatch_csr, nt_index.parallel_locate_mismatch_csr),
             (pattern_ref.brute_force, nt_index.parallel_count_pattern_csr, nt_index.parallel_locate_pattern_csr))
    for k in (0, 1):
        for ref, count, locate in paths:
            counts = count(qb, qo, k)
            off, gpos, _, mm = locate(qb, qo, k)
            for i, q in enumerate(qs):
                wc, wp, wd = ref(text, q, k, 0)
                assert np.array_equal(counts[i], wc), (q, k, counts[i], wc)
                g = gpos[off[i]:off[i + 1]].astype(np.int64)
                order = np.argsort(g, kind="stable")
                assert np.array_equal(g[order], wp) and np.array_equal(mm[off[i]:off[i + 1]][order], wd), (q, k)
    letters, classes = mr.brute_force(text, qs[0], 0, 0)[0], pattern_ref.brute_force(text, qs[0], 0, 0)[0]
    assert int(classes[0]) >= 1 and int(classes[0]) != int(letters[0])  # the inputs cannot hide a swapped table
    assert int(nt_index.parallel_count_pattern_csr(qb, qo, 0)[0, 0]) != int(nt_index.parallel_count_mismatch_csr(qb, qo, 0)[0, 0])


def test_seven_reads_halved_down_to_single_reads_equal_the_uncapped_call(nt_index, nt_text):
    qs = [bytes(q) for q in synth.sampled_queries(nt_text[0], 7, 25, 3)]
    qb, qo = pack_queries(qs)
    want = {k: _results(nt_index, qb, qo, k) for k in (1, 2)}
    assert int(want[2][1][-1]) >= 7
    os.environ["AWRY_MISMATCH_LEAF_CAP"] = "1"  # every chunk of more than one read is over capacity
    try:
        for k in (1, 2):
            got = _results(nt_index, qb, qo, k)
            assert len(got) == len(want[k]) and _same(got, want[k]), k
    finally:
        del os.environ["AWRY_MISMATCH_LEAF_CAP"]
