"""Anchors without a GPU: the two references of tests/anchor_ref.py agree with each other, the C ABI declares and exports the
entry points, and the argument / no-replica errors come back as status codes."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from awry_amd import _lib
from awry_amd.fm_index import ANCHOR_DTYPE, ERR_ARG, ERR_NO_DEVICE, BUILD_HOST, AwryError, FmIndex, pack_queries
from tests import anchor_ref as ar
from tests import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "awry_hip.h")
ENTRY_POINTS = ("awry_anchor_batch", "awry_locate_anchors_batch", "awry_dev_anchors", "awry_dev_anchors_tally")


def reference_queries(text, alphabet, rng, n_sampled, n_random):
    """sampled windows with 0..4 planted substitutions, random strings, short ones, other bytes"""
    letters = synth.NT if alphabet == 0 else synth.AA
    n = len(text) - 1
    qs = []
    for _ in range(n_sampled):
        L = int(rng.integers(1, 90))
        p = int(rng.integers(0, n - L))
        q = bytearray(text[p:p + L])
        for _ in range(int(rng.integers(0, 5))):
            q[int(rng.integers(0, L))] = int(letters[rng.integers(0, len(letters))])
        qs.append(bytes(q))
    for _ in range(n_random):
        qs.append(bytes(letters[rng.integers(0, len(letters), size=int(rng.integers(1, 60)))]))
    qs += [b"N", b"NNNN", b"acgu", b"ACGTRYKMSWBDHVN"] if alphabet == 0 else [b"X", b"mkvB", b"W", b"BZJUO"]
    return qs


@pytest.mark.parametrize("alphabet,n,seed", [(0, 20_000, 31), (1, 5_000, 32)])
def test_definition_and_stepping_references_agree(oracle, alphabet, n, seed):
    text, st, hd = synth.make_text(n, alphabet, seed, 4, 0.02)
    oi = oracle.OracleIndex.from_text(text, alphabet, 8, 0, st, hd)
    ctext = ar.canonical_text(text, alphabet)
    qs = reference_queries(text, alphabet, np.random.default_rng(seed), 60, 30)
    total = 0
    for skip in (0, 1):
        for min_len in (1, 5):
            for q in qs:
                a = ar.anchors_definition(ctext, oi, q, alphabet, min_len, skip)
                b = ar.anchors_stepping(oi, q, alphabet, min_len, skip)
                assert a == b, (q, min_len, skip)
                assert all(x[0] > y[0] for x, y in zip(a, a[1:])), q  # right to left
                total += len(a)
    assert total > 4 * len(qs)  # (the batch does cut queries into several anchors)
    for bad in (b"", b"AC$", bytes([65, 200])):
        with pytest.raises(ValueError):
            ar.anchors_stepping(oi, bad, alphabet)
        with pytest.raises(ValueError):
            ar.anchors_definition(ctext, oi, bad, alphabet)


def test_whole_match_is_one_anchor_in_both_references(oracle):
    text, st, hd = synth.make_text(3_000, 0, 33, 1, 0.0)
    oi = oracle.OracleIndex.from_text(text, 0, 8, 0, st, hd)
    ctext = ar.canonical_text(text, 0)
    q = bytes(text[100:180])
    sp, ep = oi.search_range(q)
    for skip in (0, 1):
        assert ar.anchors_definition(ctext, oi, q, 0, 1, skip) == [(0, 80, sp, ep - sp + 1)]
        assert ar.anchors_stepping(oi, q, 0, 1, skip) == [(0, 80, sp, ep - sp + 1)]
    assert ar.anchors_stepping(oi, q, 0, 81, 0) == []
    # a text without N: a query N is an absent letter and is passed over
    assert ar.anchors_stepping(oi, b"NNN", 0) == [] and ar.anchors_definition(ctext, oi, b"NNN", 0) == []
    got = ar.anchors_stepping(oi, q[:40] + b"N" + q[41:], 0)
    assert [(b, ln) for b, ln, _, _ in got][0] == (41, 39) and got[-1][0] == 0


def test_header_declares_and_library_exports_the_entry_points():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"typedef\s+struct\s*\{\s*uint32_t\s+q_begin\s*,\s*q_len\s*;\s*uint64_t\s+start_row\s*,\s*count\s*;\s*\}\s*awry_anchor_t\s*;", src)
    L = _lib.load_library()
    for name in ENTRY_POINTS:
        assert name in _lib.header_symbols(), name
        assert getattr(L, name) is not None, name


def test_anchor_record_is_24_bytes_in_c_ctypes_and_numpy(tmp_path):
    assert C.sizeof(_lib.Anchor) == 24 and ANCHOR_DTYPE.itemsize == 24
    for f, o in (("q_begin", 0), ("q_len", 4), ("start_row", 8), ("count", 16)):
        assert getattr(_lib.Anchor, f).offset == o and ANCHOR_DTYPE.fields[f][1] == o
    src = tmp_path / "size.c"
    src.write_text('#include <stddef.h>\n#include "awry_hip.h"\n_Static_assert(sizeof(awry_anchor_t) == 24, "size");\n'
                   '_Static_assert(offsetof(awry_anchor_t, start_row) == 8 && offsetof(awry_anchor_t, count) == 16, "layout");\nint main(void) { return 0; }\n')
    subprocess.check_call(["gcc", "-std=c11", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


@pytest.fixture(scope="module")
def hostonly_index():
    text, st, hd = synth.make_text(2_000, 0, 34, 1, 0.0)
    return FmIndex.from_text(text, 0, 8, 0, st, hd, build_device=BUILD_HOST)  # no set_devices: no replica


def test_without_replicas_the_batch_calls_return_no_device(hostonly_index):
    qb, qo = pack_queries([b"ACGT", b"GATTACA"])
    for call in (lambda: hostonly_index.parallel_anchors_csr(qb, qo, 1, 0), lambda: hostonly_index.parallel_locate_anchors_csr(qb, qo, 10),
                 lambda: hostonly_index.anchors_string(b"ACGT"), lambda: hostonly_index.dev_anchors(None, None, 0, 1, 0, None)):
        with pytest.raises(AwryError) as e:
            call()
        assert e.value.code == ERR_NO_DEVICE


def test_bad_min_len_skip_and_max_hits_are_argument_errors(hostonly_index):
    qb, qo = pack_queries([b"ACGT"])
    bad = [lambda: hostonly_index.parallel_anchors_csr(qb, qo, 0, 0), lambda: hostonly_index.parallel_anchors_csr(qb, qo, 1, 2),
           lambda: hostonly_index.parallel_anchors_csr(qb, qo, 1, -1), lambda: hostonly_index.parallel_locate_anchors_csr(qb, qo, 0),
           lambda: hostonly_index.parallel_locate_anchors_csr(qb, qo, 5, 0, 0), lambda: hostonly_index.parallel_locate_anchors_csr(qb, qo, 5, 1, 3),
           lambda: hostonly_index.dev_anchors(None, None, 0, 0, 0, None), lambda: hostonly_index.dev_anchors(None, None, 0, 1, 2, None)]
    for call in bad:
        with pytest.raises(AwryError) as e:
            call()
        assert e.value.code == ERR_ARG
    # the out-pointers of a failed call stay as they were
    L = _lib.load_library()
    off, an = C.POINTER(C.c_uint64)(), C.POINTER(_lib.Anchor)()
    rc = L.awry_anchor_batch(hostonly_index._h, qb.ctypes.data, qo.ctypes.data_as(C.POINTER(C.c_uint64)), 1, 0, 0, C.byref(off), C.byref(an))
    assert rc == ERR_ARG and not off and not an
