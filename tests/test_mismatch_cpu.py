"""Substitution-tolerant search, CPU side: the two references of tests/mismatch_ref.py agree with each other, the library
exports the new entry points, and without a replica they fail loudly (there is no CPU search path)."""
import numpy as np
import pytest

import awry_amd
from awry_amd import _lib
from awry_amd.fm_index import ERR_ARG, ERR_NO_DEVICE, MAX_MISMATCHES, AwryError, FmIndex
from tests import mismatch_ref as mr
from tests import synth

NEW_SYMBOLS = ("awry_count_mismatch_batch", "awry_locate_mismatch_batch", "awry_dev_count_mismatch", "awry_dev_count_mismatch_tally",
               "awry_debug_rank_all")


def test_library_exports_the_mismatch_entry_points():
    L = awry_amd.load_library()
    declared = set(_lib.header_symbols())
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert hasattr(L, name), name
    assert MAX_MISMATCHES == 2


def test_variant_enumeration_sizes():
    assert len(mr.variants(b"ACGTACGTACGTACGTACGTACGTACGTACG", 1)) == 31 * 4
    assert len(mr.variants(b"ACGTACGTACGTACGTACGTACGTACGTACG", 2)) == 465 * 16
    assert len(mr.variants(b"MKV", 1, alphabet=1)) == 3 * 20
    assert mr.variants(b"acgu", 0) == [b"ACGT"]
    assert mr.variants(b"r", 0) == [b"N"]


ODD_QUERIES = {0: [b"ACGTNacgu", b"r", b"ACGTRYKMSWBDHVN", b"acgtnnnnacgt", b"UUAGC", b"AC", b"G", b"ACGTACGTACGTACGTACGTACGTACGTACG"],
               1: [b"MKVx", b"b", b"WYACD", b"mkvBZJOU", b"ACGU", b"XXX", b"L"]}


@pytest.mark.parametrize("alphabet", [0, 1])
def test_vectorised_enumerator_equals_variants(alphabet):
    """the same strings in the same order as the itertools enumerator, for N / X, lower case, U and IUPAC bytes and d > L"""
    for q in ODD_QUERIES[alphabet]:
        for d in (0, 1, 2, 3):
            a = mr.variants_array(q, d, alphabet)
            assert a.dtype == np.uint8 and a.shape[1] == len(q)
            want = mr.variants(q, d, alphabet) if d <= len(q) else []
            assert [bytes(r) for r in a] == want, (q, d)
            assert len(set(want)) == len(want)
    L, na = 31, 4
    assert len(mr.variants_array(b"A" * L, 2, 0)) == L * (L - 1) // 2 * na * na
    assert len(mr.variants_array(b"M" * 12, 2, 1)) == 66 * 400


@pytest.mark.parametrize("alphabet,n,recs,nfrac,seed", [(0, 120_000, 4, 0.02, 11), (1, 60_000, 5, 0.01, 12)])
def test_oracle_batch_reference_equals_brute_force_and_oracle_locate(oracle, alphabet, n, recs, nfrac, seed):
    """oracle_counts_batch / oracle_search_batch (chunked: max_bytes forces several oracle calls) against the definition, and
    the batch's hit lists against oracle_locate"""
    text, st, hd = synth.make_text(n, alphabet, seed, recs, nfrac)
    oi = oracle.OracleIndex.from_text(text, alphabet, 4, 0, st, hd)
    rng = np.random.default_rng(seed)
    lens = (1, 2, 3, 6, 9, 14, 31) if alphabet == 0 else (1, 2, 3, 4, 6, 9)
    qs = list(ODD_QUERIES[alphabet]) + [b""]
    for L in lens:
        qs += [bytes(q) for q in synth.sampled_queries(text, 2, L, seed + L, alphabet=alphabet)]
        qs += [bytes(q) for q in synth.random_queries(1, L, alphabet, seed + L)]
        q = bytearray(synth.sampled_queries(text, 1, L, seed + 50 + L, alphabet=alphabet)[0])
        for _ in range(min(2, L)):
            j = int(rng.integers(0, L))
            q[j] = ord("C") if q[j] != ord("C") else ord("A")
        qs.append(bytes(q))
    qs += [bytes(text[s - 4:s + 5]) for s in st[1:]] + [bytes(text[st[1] - 2:st[1] + 3]).lower()]
    amb = np.flatnonzero(text[:-1] == (ord("N") if alphabet == 0 else ord("X")))
    qs.append(bytes(text[int(amb[0]) - 5:int(amb[0]) + 3]))
    for k in (0, 1, 2):
        counts, leaves, off, g, p, d = mr.oracle_search_batch(oi, qs, k, alphabet, 4, True, max_bytes=20_000)
        c2, l2 = mr.oracle_counts_batch(oi, qs, k, alphabet, 4)
        assert np.array_equal(c2, counts) and np.array_equal(l2, leaves)
        assert counts.shape == (len(qs), k + 1) and int(off[-1]) == len(g) == len(p) == len(d)
        for i, q in enumerate(qs):
            want, pos, dist = mr.brute_force(text, q, k, alphabet)
            assert np.array_equal(counts[i], want), (q, k, counts[i], want)
            a, b = int(off[i]), int(off[i + 1])
            order = np.argsort(g[a:b], kind="stable")
            assert np.array_equal(g[a:b][order].astype(np.int64), pos) and np.array_equal(d[a:b][order], dist), (q, k)
            if len(q) and (i % 3 == 0 or len(q) <= 3):
                og, op, od = mr.oracle_locate(oi, q, k, alphabet)
                assert np.array_equal(g[a:b], og) and np.array_equal(p[a:b], op) and np.array_equal(d[a:b], od), (q, k)
                assert leaves[i] <= len(og) and (leaves[i] > 0) == (len(og) > 0)
    assert int(leaves.max()) > 100


@pytest.mark.parametrize("alphabet,n,recs,nfrac,seed", [(0, 60_000, 3, 0.02, 1), (0, 20_000, 1, 0.0, 2), (1, 30_000, 4, 0.01, 3)])
def test_brute_force_agrees_with_variant_enumeration(oracle, alphabet, n, recs, nfrac, seed):
    text, st, hd = synth.make_text(n, alphabet, seed, recs, nfrac)
    oi = oracle.OracleIndex.from_text(text, alphabet, 4, 0, st, hd)
    rng = np.random.default_rng(seed)
    L = 9 if alphabet == 0 else 5
    queries = list(synth.random_queries(3, L, alphabet, seed)) + list(synth.sampled_queries(text, 3, L, seed, alphabet=alphabet))
    # planted substitutions and a window across a record join / N run
    q = bytearray(synth.sampled_queries(text, 1, L, seed + 7, alphabet=alphabet)[0])
    q[rng.integers(0, L)] = ord("C") if q[0] != ord("C") else ord("A")
    queries.append(bytes(q))
    if recs > 1:
        queries.append(bytes(text[st[1] - 3: st[1] - 3 + L]).lower())
    for k in (0, 1, 2):
        for q in queries:
            q = bytes(q)
            want, pos, dist = mr.brute_force(text, q, k, alphabet)
            assert np.array_equal(mr.oracle_counts(oi, q, k, alphabet), want), (q, k)
            g, p, d = mr.oracle_locate(oi, q, k, alphabet)
            order = np.argsort(g, kind="stable")
            assert np.array_equal(g[order].astype(np.int64), pos), (q, k)
            assert np.array_equal(d[order], dist), (q, k)


def test_k_at_least_query_length_matches_every_window(oracle):
    text, st, hd = synth.make_text(5_000, 0, 4, 2, 0.0)
    want, pos, _ = mr.brute_force(text, b"AC", 2)
    assert int(want.sum()) == len(text) - 2  # every window of 2 letters without '$'


def test_mismatch_calls_need_a_replica_and_a_valid_k():
    text, st, hd = synth.make_text(500, 0, 1)
    ix = FmIndex.from_text(text, 0, 8, 0, st, hd)
    for call in (lambda k: ix.parallel_count_mismatch(["ACGT"], k), lambda k: ix.parallel_locate_mismatch_csr(*awry_amd.fm_index.pack_queries(["ACGT"]), k)):
        with pytest.raises(AwryError) as e:
            call(1)
        assert e.value.code == ERR_NO_DEVICE
        for bad in (3, -1):
            with pytest.raises(AwryError) as e:
                call(bad)
            assert e.value.code == ERR_ARG
    L = awry_amd.load_library()
    assert L.awry_dev_count_mismatch(ix._h, 0, None, None, 0, 1, None, None, None) == ERR_NO_DEVICE
    assert L.awry_dev_count_mismatch(ix._h, 0, None, None, 0, 3, None, None, None) == ERR_ARG
