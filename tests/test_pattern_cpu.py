"""Class-pattern search, CPU side: the library's class table against the one written out in tests/pattern_ref.py, the
brute-force reference against the mismatch reference (plain letters) and against the oracle's exact counts of the expanded
strings (k = 0), the exported entry points, and the loud failure without a replica (there is no CPU search path)."""
import numpy as np
import pytest

import awry_amd
from awry_amd import _lib
from awry_amd.fm_index import ERR_ARG, ERR_NO_DEVICE, AwryError, FmIndex, pack_queries
from tests import mismatch_ref as mr
from tests import pattern_ref as pr
from tests import synth

NEW_SYMBOLS = ("awry_pattern_class", "awry_count_pattern_batch", "awry_locate_pattern_batch", "awry_dev_count_pattern",
               "awry_dev_count_pattern_tally")


def test_pattern_class_equals_the_reference_table():
    L = awry_amd.load_library()
    for alphabet in (0, 1):
        want = pr.class_table(alphabet)
        got = np.array([L.awry_pattern_class(alphabet, b) for b in range(256)], np.uint32)
        assert np.array_equal(got, want), (alphabet, [chr(b) for b in np.flatnonzero(got != want)])
        assert all(awry_amd.pattern_class(alphabet, chr(b)) == int(want[b]) for b in range(1, 128))
        amb = 4 if alphabet == 0 else 20
        assert not (want & np.uint32((1 << amb) | 1)).any()  # no class holds the sentinel or the ambiguity symbol
    assert L.awry_pattern_class(2, ord("A")) == 0
    nt, aa = pr.class_table(0), pr.class_table(1)
    assert int((nt != 0).sum()) == 2 * 16 and int((aa != 0).sum()) == 2 * 24
    assert nt[ord("N")] == 0b101110 and nt[ord("u")] == nt[ord("T")] == 1 << 5 and nt[ord("X")] == 0
    assert bin(int(aa[ord("X")])).count("1") == 20 and aa[ord("U")] == 0 and aa[ord("O")] == 0 and aa[ord("*")] == 0


def test_library_exports_the_pattern_entry_points():
    L = awry_amd.load_library()
    declared = set(_lib.header_symbols())
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert hasattr(L, name), name


@pytest.mark.parametrize("alphabet,n,recs,nfrac,seed", [(0, 30_000, 3, 0.02, 21), (1, 20_000, 3, 0.01, 22)])
def test_brute_force_equals_the_mismatch_reference_for_plain_letters(alphabet, n, recs, nfrac, seed):
    text, st, _ = synth.make_text(n, alphabet, seed, recs, nfrac)
    qs = []
    for L in (1, 2, 3, 5, 9, 14, 31):
        qs += [bytes(q) for q in synth.sampled_queries(text, 2, L, seed + L, alphabet=alphabet)]
        qs += [bytes(q) for q in synth.random_queries(1, L, alphabet, seed + L)]
    plain = (pr.class_table(alphabet) & (pr.class_table(alphabet) - 1)) == 0
    qs += [bytes(text[st[1] - 4:st[1] + 5]), bytes(qs[-2]).lower()]
    qs = [bytes(b for b in q if pr.class_table(alphabet)[b] != 0 and plain[b]) for q in qs]
    qs = [q for q in qs if q]
    if alphabet == 0:
        qs.append(b"acguACGU")
    for k in (0, 1, 2):
        for q in qs:
            a, b = pr.brute_force(text, q, k, alphabet), mr.brute_force(text, q, k, alphabet)
            assert all(np.array_equal(x, y) for x, y in zip(a, b)), (q, k)


@pytest.mark.parametrize("alphabet,n,recs,nfrac,seed", [(0, 60_000, 3, 0.02, 31), (1, 40_000, 4, 0.01, 32)])
def test_k0_brute_force_equals_oracle_counts_of_the_expanded_strings(oracle, alphabet, n, recs, nfrac, seed):
    text, st, hd = synth.make_text(n, alphabet, seed, recs, nfrac)
    oi = oracle.OracleIndex.from_text(text, alphabet, 4, 0, st, hd)
    rng = np.random.default_rng(seed)
    pats = [b"RYRYRY", b"GANTC", b"nnGGnn", b"ACGWSKM", b"BDHVAC"] if alphabet == 0 else [b"BZJ", b"mXk", b"AXXL", b"JJBZZB", b"CxxC"]
    for L, c in ((4, 1), (6, 2), (9, 3), (12, 4), (12, 6), (20, 6)):
        w = bytes(synth.sampled_queries(text, 1, L, seed + L + c, alphabet=alphabet)[0])
        positions = rng.choice(L, c, replace=False)
        hold = rng.random(c) < 0.7
        if alphabet == 1:  # keep the expansion small: X (20 residues) at two positions at the most
            hold[2:] = False
        pats.append(pr.replace_with_classes(w, positions, hold, alphabet, rng))
    for p in pats:
        assert pr.class_positions(p, alphabet) <= 6
        strings = pr.expand(p, alphabet)
        assert 1 <= len(strings) <= 200_000, p
        c, _ = oi.parallel_count(*pack_queries(strings), 4)
        want, pos, d = pr.brute_force(text, p, 0, alphabet)
        assert int(c.sum()) == int(want[0]) == len(pos) and not d.any(), p
    assert sum(int(pr.brute_force(text, p, 0, alphabet)[0][0]) for p in pats) > 50


def test_ordered_hits_equals_the_mismatch_order_for_plain_letters(oracle):
    text, st, hd = synth.make_text(40_000, 0, 33, 2, 0.01)
    oi = oracle.OracleIndex.from_text(text, 0, 4, 0, st, hd)
    for q in [bytes(x) for x in synth.sampled_queries(text, 2, 8, 34)] + [b"ACGTA"]:
        for k in (0, 1, 2):
            a, b = pr.ordered_hits(oi, text, q, k, 0), mr.oracle_locate(oi, q, k, 0)
            assert all(np.array_equal(x, y) for x, y in zip(a, b)), (q, k)


def test_pattern_calls_need_a_replica_and_a_valid_k():
    text, st, hd = synth.make_text(500, 0, 1)
    ix = FmIndex.from_text(text, 0, 8, 0, st, hd)
    for call in (lambda k: ix.parallel_count_pattern(["GANTC"], k), lambda k: ix.parallel_locate_pattern_csr(*pack_queries(["GANTC"]), k)):
        with pytest.raises(AwryError) as e:
            call(1)
        assert e.value.code == ERR_NO_DEVICE
        for bad in (3, -1):
            with pytest.raises(AwryError) as e:
                call(bad)
            assert e.value.code == ERR_ARG
    L = awry_amd.load_library()
    assert L.awry_dev_count_pattern(ix._h, 0, None, None, 0, 1, None, None, None) == ERR_NO_DEVICE
    assert L.awry_dev_count_pattern(ix._h, 0, None, None, 0, 3, None, None, None) == ERR_ARG
