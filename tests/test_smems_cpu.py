"""SMEMs without a GPU: the two references of tests/smem_ref.py agree with each other and with the header's three conditions,
the C ABI declares and exports the entry points, the argument / no-replica errors come back as status codes, and the C++
mirror's methods compile."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from awry_amd import _lib
from awry_amd.fm_index import ERR_ARG, ERR_NO_DEVICE, BUILD_HOST, AwryError, FmIndex, pack_queries
from tests import anchor_ref as ar
from tests import smem_ref as sr
from tests import synth
from tests.test_anchors_cpu import reference_queries

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("awry_smem_batch", "awry_locate_smems_batch", "awry_dev_smems", "awry_dev_smems_tally")


@pytest.mark.parametrize("alphabet,n,seed", [(0, 20_000, 31), (1, 5_000, 32)])
def test_definition_and_oracle_references_agree(oracle, alphabet, n, seed):
    text, st, hd = synth.make_text(n, alphabet, seed, 4, 0.02)
    oi = oracle.OracleIndex.from_text(text, alphabet, 8, 0, st, hd)
    ctext = ar.canonical_text(text, alphabet)
    qs = reference_queries(text, alphabet, np.random.default_rng(seed), 60, 30)
    total = differs = 0
    for q in qs:
        a = sr.smems_definition(ctext, oi, q, alphabet, 1)
        assert a == sr.smems_oracle(oi, q, alphabet, 1), q
        assert all(x[0] > y[0] and x[0] + x[1] > y[0] + y[1] for x, y in zip(a, a[1:])), q  # descending begins and descending ends
        assert len(a) <= len(q)
        cq = ar.canonical(q, alphabet)
        occurs = lambda b, e: ctext.find(cq[b:e]) >= 0
        assert all(sr.is_smem(occurs, len(cq), b, b + ln) for b, ln, _, _ in a), q
        # every letter that occurs is covered; no SMEM holds another
        covered = set(j for b, ln, _, _ in a for j in range(b, b + ln))
        assert covered == set(j for j in range(len(cq)) if occurs(j, j + 1)), q
        for min_len in (5,):
            assert sr.smems_definition(ctext, oi, q, alphabet, min_len) == [x for x in a if x[1] >= min_len]
            assert sr.smems_oracle(oi, q, alphabet, min_len) == [x for x in a if x[1] >= min_len]
        # the first SMEM is the first skip = 0 anchor: both are the longest match that ends at the last letter that occurs
        anchors = ar.anchors_definition(ctext, oi, q, alphabet, 1, 0)
        assert a[:1] == anchors[:1], q
        differs += a != anchors
        total += len(a)
    assert total > 4 * len(qs) and differs > len(qs) // 4  # (the batch does have several SMEMs per query, and they are not the anchors)
    for bad in (b"", b"AC$", bytes([65, 200])):
        with pytest.raises(ValueError):
            sr.smems_oracle(oi, bad, alphabet)
        with pytest.raises(ValueError):
            sr.smems_definition(ctext, oi, bad, alphabet)


def test_whole_match_and_absent_letter_in_both_references(oracle):
    text, st, hd = synth.make_text(3_000, 0, 33, 1, 0.0)
    oi = oracle.OracleIndex.from_text(text, 0, 8, 0, st, hd)
    ctext = ar.canonical_text(text, 0)
    q = bytes(text[100:180])
    sp, ep = oi.search_range(q)
    assert sr.smems_definition(ctext, oi, q, 0) == [(0, 80, sp, ep - sp + 1)] == sr.smems_oracle(oi, q, 0)
    assert sr.smems_oracle(oi, q, 0, 81) == []
    # a text without N: a query N is an absent letter, belongs to no SMEM and splits the matches around it
    assert sr.smems_oracle(oi, b"NNN", 0) == [] and sr.smems_definition(ctext, oi, b"NNN", 0) == []
    got = sr.smems_oracle(oi, q[:40] + b"N" + q[41:], 0)
    assert [(b, ln) for b, ln, _, _ in got] == [(41, 39), (0, 40)]


def test_header_declares_and_library_exports_the_entry_points():
    L = _lib.load_library()
    for name in ENTRY_POINTS:
        assert name in _lib.header_symbols(), name
        assert getattr(L, name) is not None, name


@pytest.fixture(scope="module")
def hostonly_index():
    text, st, hd = synth.make_text(2_000, 0, 34, 1, 0.0)
    return FmIndex.from_text(text, 0, 8, 0, st, hd, build_device=BUILD_HOST)  # no set_devices: no replica


def test_without_replicas_the_batch_calls_return_no_device(hostonly_index):
    qb, qo = pack_queries([b"ACGT", b"GATTACA"])
    for call in (lambda: hostonly_index.parallel_smems_csr(qb, qo, 1), lambda: hostonly_index.parallel_locate_smems_csr(qb, qo, 10),
                 lambda: hostonly_index.smems_string(b"ACGT"), lambda: hostonly_index.dev_smems(None, None, 0, 1, None),
                 lambda: hostonly_index.dev_smems_tally(None, None, 0, 1, None, None)):
        with pytest.raises(AwryError) as e:
            call()
        assert e.value.code == ERR_NO_DEVICE


def test_bad_min_len_and_max_hits_are_argument_errors(hostonly_index):
    qb, qo = pack_queries([b"ACGT"])
    bad = [lambda: hostonly_index.parallel_smems_csr(qb, qo, 0), lambda: hostonly_index.parallel_locate_smems_csr(qb, qo, 0),
           lambda: hostonly_index.parallel_locate_smems_csr(qb, qo, 5, 0), lambda: hostonly_index.dev_smems(None, None, 0, 0, None),
           lambda: hostonly_index.dev_smems_tally(None, None, 0, 0, None, None)]
    for call in bad:
        with pytest.raises(AwryError) as e:
            call()
        assert e.value.code == ERR_ARG
    # the out-pointers of a failed call stay as they were
    L = _lib.load_library()
    u64p = C.POINTER(C.c_uint64)
    off, an, hoff, hits, gp = u64p(), C.POINTER(_lib.Anchor)(), u64p(), C.POINTER(_lib.Pos)(), u64p()
    rc = L.awry_smem_batch(hostonly_index._h, qb.ctypes.data, qo.ctypes.data_as(u64p), 1, 0, C.byref(off), C.byref(an))
    assert rc == ERR_ARG and not off and not an
    for min_len, max_hits in ((0, 5), (1, 0)):
        rc = L.awry_locate_smems_batch(hostonly_index._h, qb.ctypes.data, qo.ctypes.data_as(u64p), 1, min_len, max_hits, C.byref(off), C.byref(an),
                                       C.byref(hoff), C.byref(hits), C.byref(gp))
        assert rc == ERR_ARG and not off and not an and not hoff and not hits and not gp


def test_cpp_mirror_methods_compile(tmp_path):
    src = tmp_path / "smems.cpp"
    src.write_text('#include <string>\n#include <vector>\n#include "awry.hpp"\n'
                   "uint64_t use(awry::FmIndex& ix) {\n"
                   '  std::vector<std::string> qs{"ACGT", "GATTACA"};\n'
                   "  uint64_t s = 0;\n"
                   "  for (auto& per : ix.parallel_smems(qs, 12))\n"
                   "    for (const awry::FmIndex::Anchor& a : per) s += a.q_begin + a.q_len + a.rows.start_ptr;\n"
                   "  for (auto& per : ix.parallel_locate_smems(qs, 50, 12))\n"
                   "    for (const awry::FmIndex::LocatedAnchor& la : per) s += la.anchor.q_len + la.hits.size();\n"
                   "  return s;\n}\n")
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"), str(src)])
