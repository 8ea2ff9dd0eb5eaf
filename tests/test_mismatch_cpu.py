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
