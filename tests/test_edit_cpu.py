"""Locate within k edits without a GPU: tests/edit_ref.py equals a plain cell-by-cell DP, equals the oracle's exact locate at
k = 0, and the device's plan (pieces, diagonals, merged runs, cut windows) run in Python equals the global rule; the C ABI
declares and exports the entry points, the argument / no-replica errors come back as status codes, and the C++ mirror's method
compiles."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from awry_amd import _lib
from awry_amd.fm_index import ERR_ARG, ERR_NO_DEVICE, BUILD_HOST, AwryError, FmIndex, pack_queries
from tests import edit_ref as er
from tests import mismatch_ref as mr
from tests import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("awry_locate_edit_batch", "awry_dev_edit_windows", "awry_dev_edit_windows_tally")


def plain_dp(tsym, qsym):
    """D(s) by the textbook table, one start at a time: the cells of q against T[s .. s + 2L) (a best alignment ends by s + 2L)"""
    n, L = len(tsym), len(qsym)
    out = []
    for s in range(n):
        m = min(n, s + 2 * L) - s
        prev = list(range(m + 1))  # edit_distance(empty, T[s..s+j)) = j
        for i in range(1, L + 1):
            cur = [i] + [0] * m
            for j in range(1, m + 1):
                cur[j] = min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (qsym[i - 1] != tsym[s + j - 1]))
            prev = cur
        out.append(min(prev))
    return np.array(out, np.int32)


def edited(rng, q, e, letters):
    """e random edits (substitution, insertion, deletion) on the bytes q"""
    q = bytearray(q)
    for _ in range(e):
        kind = int(rng.integers(0, 3))
        j = int(rng.integers(0, len(q)))
        if kind == 0:
            q[j] = int(letters[(int(np.nonzero(letters == q[j])[0][0]) + 1) % len(letters)]) if q[j] in bytes(letters) else int(letters[0])
        elif kind == 1:
            q.insert(j, int(letters[rng.integers(0, len(letters))]))
        elif len(q) > 1:
            del q[j]
    return bytes(q)


def small_cases(rng, alphabet, count, nmax=300, Lmax=40):
    """(text with '$', query, k): alphabets of 2..4 letters (or the amino letters), homopolymer and tandem runs, k <= 3, reads
    at the text's two ends"""
    out = []
    for _ in range(count):
        if alphabet == 0:
            letters = synth.NT[:int(rng.integers(2, 5))]
        else:
            letters = synth.AA[:int(rng.integers(2, 21))]
        n = int(rng.integers(30, nmax))
        body = letters[rng.integers(0, len(letters), size=n)].copy()
        if rng.random() < 0.5:  # a homopolymer or short-period tandem run
            p, ln, per = int(rng.integers(0, n - 20)), int(rng.integers(8, 20)), int(rng.integers(1, 4))
            body[p:p + ln] = np.resize(letters[rng.integers(0, len(letters), size=per)], ln)
        if rng.random() < 0.3:
            body[int(rng.integers(0, n))] = ord("N") if alphabet == 0 else ord("X")
        k = int(rng.integers(0, 4))
        L = int(rng.integers(k + 1, Lmax + 1))
        where = rng.random()
        p = 0 if where < 0.2 else (max(0, n - L) if where < 0.4 else int(rng.integers(0, max(1, n - L))))
        q = edited(rng, bytes(body[p:p + L]), int(rng.integers(0, k + 2)), letters)
        while len(q) <= k:
            q += bytes(letters[:1])
        out.append((np.concatenate([body, np.frombuffer(b"$", np.uint8)]), q, k))
    return out


@pytest.mark.parametrize("alphabet,seed", [(0, 41), (1, 42)])
def test_reference_equals_a_plain_dp(alphabet, seed):
    rng = np.random.default_rng(seed)
    for text, q, k in small_cases(rng, alphabet, 12, 150, 25):
        t = er.Text(text, alphabet)
        qs = mr.to_symbols(q, alphabet)
        assert np.array_equal(er.distances(t.sym, qs), plain_dp([int(v) for v in t.sym], [int(v) for v in qs])), (bytes(text), q)


def test_hit_rule_on_a_hand_made_profile():
    D = np.array([3, 2, 2, 3, 1, 0, 1, 5, 2], np.int32)
    p, d = er.hits_of(D, 2)
    assert list(p) == [1, 2, 5, 8] and list(d) == [2, 2, 0, 2]  # a plateau whole, a minimum once, the last start against D(n) = +inf
    assert list(er.hits_of(D, 2, 2, 6)[0]) == [2, 5]
    assert er.pieces(10, 2) == [(0, 3), (3, 6), (6, 10)] and er.pieces(3, 2) == [(0, 1), (1, 2), (2, 3)]


@pytest.mark.parametrize("alphabet,n,seed", [(0, 20_000, 43), (1, 5_000, 44)])
def test_at_k0_the_reference_is_the_oracles_locate(oracle, alphabet, n, seed):
    text, st, hd = synth.make_text(n, alphabet, seed, 4, 0.02)
    oi = oracle.OracleIndex.from_text(text, alphabet, 8, 0, st, hd)
    t = er.Text(text, alphabet)
    rng = np.random.default_rng(seed)
    qs = [bytes(text[p:p + L]) for L in (1, 2, 5, 12, 40) for p in rng.integers(0, n - 40, size=6)]
    qs += [b"N" * 3 if alphabet == 0 else b"X" * 3, bytes(text[:9]), bytes(text[n - 9:n])]
    for q in qs:
        g, _ = oi.locate_string(q)
        p, d = er.hits_of(t.D(q), 0)
        assert sorted(int(v) for v in g) == list(p), q
        assert not d.any()
        assert er.candidates(t.ctext, q, 0, alphabet) == len(g)


@pytest.mark.parametrize("alphabet,seed,count", [(0, 45, 200), (1, 46, 60)])
def test_the_window_pipeline_equals_the_global_rule(alphabet, seed, count):
    rng = np.random.default_rng(seed)
    nonempty = 0
    for text, q, k in small_cases(rng, alphabet, count):
        t = er.Text(text, alphabet)
        p, d = er.hits_of(t.D(q), k)
        want = list(zip((int(v) for v in p), (int(v) for v in d)))
        assert er.window_pipeline(t, q, k) == want, (bytes(text), q, k)
        wins = er.windows_of(t.ctext, t.n, q, k, alphabet)
        assert all(a + c <= b for (a, c), (b, _) in zip(wins, wins[1:]))  # owned ranges are disjoint and ascending
        nonempty += bool(want)
    assert nonempty > count // 2


def test_header_declares_and_library_exports_the_entry_points():
    L = _lib.load_library()
    for name in ENTRY_POINTS:
        assert name in _lib.header_symbols(), name
        assert getattr(L, name) is not None, name
    header = open(os.path.join(ROOT, "include", "awry_hip.h")).read()
    for word in ("AWRY_MAX_EDITS = 8", "AWRY_EDIT_MAX_LEN = 256", "AWRY_Q_CANDIDATE_CAP = 7"):
        assert word in header, word


@pytest.fixture(scope="module")
def hostonly_index():
    text, st, hd = synth.make_text(2_000, 0, 47, 1, 0.0)
    return FmIndex.from_text(text, 0, 8, 0, st, hd, build_device=BUILD_HOST)  # no set_devices: no replica


def test_without_replicas_the_calls_return_no_device(hostonly_index):
    qb, qo = pack_queries([b"ACGTACGT", b"GATTACA"])
    for call in (lambda: hostonly_index.parallel_locate_edit_csr(qb, qo, 1, 100), lambda: hostonly_index.parallel_locate_edit([b"ACGT"], 0, 5),
                 lambda: hostonly_index.locate_string_edit(b"ACGT", 1, 5), lambda: hostonly_index.count_string_edit(b"ACGT", 1, 5),
                 lambda: hostonly_index.dev_edit_windows(None, None, None, None, None, 0, 1, None),
                 lambda: hostonly_index.dev_edit_windows_tally(None, None, None, None, None, 0, 1, None, None)):
        with pytest.raises(AwryError) as e:
            call()
        assert e.value.code == ERR_NO_DEVICE


def test_bad_max_edits_and_a_missing_cap_are_argument_errors(hostonly_index):
    qb, qo = pack_queries([b"ACGTACGTACGT"])
    bad = [lambda: hostonly_index.parallel_locate_edit_csr(qb, qo, -1, 100), lambda: hostonly_index.parallel_locate_edit_csr(qb, qo, 9, 100),
           lambda: hostonly_index.parallel_locate_edit_csr(qb, qo, 1, 0), lambda: hostonly_index.dev_edit_windows(None, None, None, None, None, 0, 9, None),
           lambda: hostonly_index.dev_edit_windows_tally(None, None, None, None, None, 0, -1, None, None)]
    for call in bad:
        with pytest.raises(AwryError) as e:
            call()
        assert e.value.code == ERR_ARG
    # the out-pointers of a failed call stay as they were
    L = _lib.load_library()
    u64p, u8p = C.POINTER(C.c_uint64), C.POINTER(C.c_uint8)
    for k, cap in ((-1, 100), (9, 100), (1, 0)):
        off, hits, gp, ed, st = u64p(), C.POINTER(_lib.Pos)(), u64p(), u8p(), u8p()
        rc = L.awry_locate_edit_batch(hostonly_index._h, qb.ctypes.data, qo.ctypes.data_as(u64p), 1, k, cap, C.byref(off), C.byref(hits), C.byref(gp),
                                      C.byref(ed), C.byref(st))
        assert rc == ERR_ARG and not off and not hits and not gp and not ed and not st


def test_cpp_mirror_method_compiles(tmp_path):
    src = tmp_path / "edit.cpp"
    src.write_text('#include <string>\n#include <vector>\n#include "awry.hpp"\n'
                   "uint64_t use(awry::FmIndex& ix) {\n"
                   '  std::vector<std::string> qs{"ACGTACGTACGT", "GATTACAGATTACA"};\n'
                   "  uint64_t s = 0;\n"
                   "  std::vector<uint8_t> status;\n"
                   "  for (auto& per : ix.parallel_locate_edit(qs, 2, 1000, &status))\n"
                   "    for (const awry::FmIndex::EditHit& h : per) s += h.position.sequence_idx() + h.position.local_position() + h.global_position + h.edits;\n"
                   "  for (uint8_t st : status) s += st == AWRY_Q_CANDIDATE_CAP;\n"
                   "  return s + ix.parallel_locate_edit(qs, 0, 10).size();\n}\n")
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"), str(src)])
