"""Mapping on both strands without a GPU: rc() on every byte, the ranking function of tests/map_ref.py on hand-made candidate lists
(ties on every key, redundancy, MAPQ, the report cap), the C ABI, ctypes, the C++ mirror and the Rust crates agree, the argument
errors that need no device come back as status codes, and the character of the fixture reads from the reference alone."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from awry_amd import _lib
from awry_amd.fm_index import (BUILD_HOST, ERR_ARG, ERR_NO_DEVICE, MAP_DTYPE, MAP_MAX_CHAINS, MAP_SECONDARY, Q_SEED_CAP, AwryError, FmIndex,
                               pack_queries)
from tests import anchor_ref as ar
from tests import chain_align_ref as ca
from tests import map_ref as mp
from tests import mismatch_ref as mr
from tests import smem_ref as sr
from tests import synth
from tests.test_chain_align_gpu import KEY, edited_reads
from tests.test_chain_gpu import E2E_PARAMS, want_chains

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("awry_map_batch", "awry_dev_revcomp", "awry_dev_map_select")
# what tests/map_ref.py gives (computed on the CPU when the test was written): of the 200 fixture reads at (min_len, max_hits) =
# (12, 20), (A, R) = (4, 1) and band 4, the reads whose primary has the planted strand, edits <= the planted edit total, |t_begin -
# origin of the forward window| <= the indel total and MAPQ > 0: 197 of 200 (the condition is 180; the chain-align suite's 196 are
# primaries among one chain per read, these among up to four per strand)
FIXTURE = dict(placed_min=180, placed=197)


# ---- rc ---------------------------------------------------------------------------------------------------------------------------

def test_rc_on_every_byte_value_and_rc_of_rc_is_the_canonical_form():
    L = _lib.load_library()
    for b in range(256):
        idx = L.awry_symbol_index(0, b)  # the library's own table
        assert mp.index_of_ascii(b) == idx, b
        want = b"$TGCNA"[idx:idx + 1]
        assert mp.rc(bytes([b])) == want, b
    assert mp.rc(b"ACGTN") == b"NACGT" and mp.rc(b"acgu") == b"ACGT" and mp.rc(b"AC$T") == b"A$GT" and mp.rc(b"RYKM#\xff") == b"N$NNNN" and mp.rc(b"") == b""
    rng = np.random.default_rng(1)
    for _ in range(200):
        q = bytes(rng.integers(0, 256, size=int(rng.integers(0, 40)), dtype=np.uint8))
        assert mp.rc(mp.rc(q)) == mp.canonical(q) and len(mp.rc(q)) == len(q)
        a = bytes(b & 0x7F for b in q)  # (the suites' symbol table covers ASCII: a byte >= 0x80 is rejected before it is looked up)
        assert mp.canonical(a) == bytes(b"$ACGNT"[int(v)] for v in mr.to_symbols(a, 0))
    assert mp.doubled([b"AAC", b"g"]) == [b"AAC", b"GTT", b"g", b"C"]


# ---- rank, redundancy, report, MAPQ on hand-made candidate lists -----------------------------------------------------------------

def hand_made_lists():
    """-> [(name, candidates (strand, j, edits, score, t_begin, t_end), capped, {R: (records' (strand, j), primary MAPQ, kept)})]"""
    c = lambda s, j, e, sc, tb, te: (s, j, e, sc, tb, te)
    return [
        ("no candidate", [], False, {1: ([], None, 0), 2: ([], None, 0)}),
        ("one candidate", [c(0, 0, 3, 90, 100, 200)], False, {1: ([(0, 0)], 60, 1), 2: ([(0, 0)], 60, 1)}),
        ("one candidate on the reverse strand", [c(1, 2, 0, 50, 7, 108)], False, {1: ([(1, 2)], 60, 1)}),
        ("edits decide before score", [c(0, 0, 2, 50, 100, 200), c(0, 1, 1, 40, 900, 1000)], False, {1: ([(0, 1)], 10, 2), 2: ([(0, 1), (0, 0)], 10, 2)}),
        ("tie on edits: the higher score", [c(0, 0, 2, 50, 100, 200), c(1, 0, 2, 70, 900, 1000)], False, {2: ([(1, 0), (0, 0)], 0, 2)}),
        ("tie on edits and score: the forward strand", [c(1, 0, 2, 50, 100, 200), c(0, 1, 2, 50, 900, 1000)], False, {2: ([(0, 1), (1, 0)], 0, 2)}),
        ("tie down to t_begin: the smaller", [c(0, 0, 2, 50, 900, 1000), c(0, 1, 2, 50, 100, 200)], False, {2: ([(0, 1), (0, 0)], 0, 2)}),
        ("tie down to j: the smaller (both have empty spans)", [c(0, 1, 2, 50, 100, 100), c(0, 0, 2, 50, 100, 100)], False, {2: ([(0, 0), (0, 1)], 0, 2)}),
        ("same-strand overlapping spans are dropped", [c(0, 0, 1, 60, 100, 200), c(0, 1, 2, 40, 199, 260), c(0, 2, 5, 30, 200, 300)], False,
         {1: ([(0, 0)], 40, 2), 2: ([(0, 0), (0, 2)], 40, 2), 3: ([(0, 0), (0, 2)], 40, 2)}),
        ("a dropped candidate drops nothing", [c(0, 0, 1, 60, 100, 200), c(0, 1, 2, 40, 150, 260), c(0, 2, 3, 30, 250, 300)], False,
         {3: ([(0, 0), (0, 2)], 20, 2)}),
        ("touching spans do not intersect", [c(1, 0, 1, 60, 100, 200), c(1, 1, 1, 50, 200, 300)], False, {2: ([(1, 0), (1, 1)], 0, 2)}),
        ("the same span on opposite strands is kept", [c(0, 0, 0, 80, 100, 180), c(1, 0, 0, 80, 100, 180)], False,
         {1: ([(0, 0)], 0, 2), 2: ([(0, 0), (1, 0)], 0, 2)}),
        ("an empty span intersects nothing", [c(0, 0, 1, 60, 100, 200), c(0, 1, 2, 40, 150, 150)], False, {2: ([(0, 0), (0, 1)], 10, 2)}),
        ("a capped strand", [c(0, 0, 0, 80, 100, 180)], True, {1: ([(0, 0)], 0, 1)}),
        ("a capped strand, two kept", [c(0, 0, 0, 80, 100, 180), c(0, 1, 9, 80, 500, 580)], True, {2: ([(0, 0), (0, 1)], 0, 2)}),
    ] + [("e2 - e1 = %d" % d, [c(0, 0, 4, 80, 100, 180), c(1, 0, 4 + d, 80, 500, 580)], False, {1: ([(0, 0)], q, 2), 2: ([(0, 0), (1, 0)], q, 2)})
         for d, q in ((0, 0), (1, 10), (5, 50), (6, 60), (7, 60))]


def test_rank_redundancy_report_and_mapq_on_hand_made_lists():
    names = set()
    for name, cands, capped, wants in hand_made_lists():
        names.add(name)
        for R, (who, mapq, nkept) in wants.items():
            recs, kept = mp.rank_candidates(cands, capped, R)
            assert [(r[5], r[4]) for r in recs] == who and kept == nkept, (name, R, recs)
            assert len(recs) == min(R, kept)
            if recs:
                assert recs[0][6] == mapq and recs[0][7] == 0, (name, R, recs)
                assert all(r[6] == 0 and r[7] == MAP_SECONDARY for r in recs[1:]), (name, R)
                by = {(c[0], c[1]): c for c in cands}
                assert all((r[0], r[1], r[2], r[3]) == (by[(r[5], r[4])][4], by[(r[5], r[4])][5], by[(r[5], r[4])][2], by[(r[5], r[4])][3]) for r in recs)
            # the order of the input list changes nothing: the order is total
            assert mp.rank_candidates(cands[::-1], capped, R) == (recs, kept), name
    assert len(names) == 20
    # R below, equal to and above the number kept
    cands = [(s, j, 2 * j + s, 50, 1000 * (2 * j + s), 1000 * (2 * j + s) + 100) for s in (0, 1) for j in range(3)]
    for R in (1, 5, 6, 7, 16):
        recs, kept = mp.rank_candidates(cands, False, R)
        assert kept == 6 and [r[2] for r in recs] == list(range(min(R, 6))) and recs[0][6] == 10
    # candidates_of: only status OK, only the first A of a strand
    per = [[(50, ca.ALN_OK, 1, 2, 0), (40, ca.ALN_SKEW, 3, 4, 0), (30, ca.ALN_OK, 5, 6, 1)], [(20, ca.ALN_BAD_CHAIN, 0, 0, 0), (10, ca.ALN_OK, 7, 8, 2)]]
    assert mp.candidates_of(per, 8) == [(0, 0, 0, 50, 1, 2), (0, 2, 1, 30, 5, 6), (1, 1, 2, 10, 7, 8)]
    assert mp.candidates_of(per, 2) == [(0, 0, 0, 50, 1, 2), (1, 1, 2, 10, 7, 8)] and mp.candidates_of(per, 1) == [(0, 0, 0, 50, 1, 2)]


# ---- declarations ---------------------------------------------------------------------------------------------------------------------

def test_header_ctypes_cpp_mirror_and_rust_agree():
    L = _lib.load_library()
    for name in ENTRY_POINTS:
        assert name in _lib.header_symbols(), name
        assert getattr(L, name) is not None, name
    header = open(os.path.join(ROOT, "include", "awry_hip.h")).read()
    for word in ("AWRY_MAP_MAX_CHAINS = 8", "AWRY_MAP_SECONDARY = 1",
                 "typedef struct { uint64_t t_begin, t_end; uint32_t edits, chain_score, chain_index; uint8_t strand, mapq; uint16_t flags; } awry_map_t;"):
        assert word in header, word
    assert "Forward strand only" not in header and "awry_map_batch (below) maps both" in header
    assert (MAP_MAX_CHAINS, MAP_SECONDARY) == (8, 1) == (mp.MAP_MAX_CHAINS, mp.MAP_SECONDARY)
    assert C.sizeof(_lib.Map) == 32 == MAP_DTYPE.itemsize == mp.MAP_NP.itemsize
    assert [(n, getattr(_lib.Map, n).offset) for n, _ in _lib.Map._fields_] == [(n, MAP_DTYPE.fields[n][1]) for n in MAP_DTYPE.names]
    assert [(n, MAP_DTYPE.fields[n][1]) for n in MAP_DTYPE.names] == [(n, mp.MAP_NP.fields[n][1]) for n in mp.MAP_NP.names]
    assert [MAP_DTYPE.fields[n][1] for n in MAP_DTYPE.names] == [0, 8, 16, 20, 24, 28, 29, 30]
    src = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in ENTRY_POINTS:
        args = re.search(r"\b%s\s*\(([^)]*)\)" % name, src).group(1)
        assert len(args.split(",")) == len(getattr(L, name).argtypes), name
    rust = open(os.path.join(ROOT, "rust", "awry-hip-sys", "src", "lib.rs")).read()
    for word in ("pub struct awry_map_t {\n    pub t_begin: u64,\n    pub t_end: u64,\n    pub edits: u32,\n    pub chain_score: u32,\n    pub chain_index: u32,\n"
                 "    pub strand: u8,\n    pub mapq: u8,\n    pub flags: u16,\n}", "pub fn awry_map_batch(", "pub fn awry_dev_revcomp(", "pub fn awry_dev_map_select("):
        assert word in rust, word
    safe = open(os.path.join(ROOT, "rust", "awry", "src", "fm_index.rs")).read()
    assert "pub fn parallel_map<'a>(" in safe and "sys::awry_map_batch(" in safe
    hpp = open(os.path.join(ROOT, "include", "awry.hpp")).read()
    assert "parallel_map(" in hpp and "awry_map_batch(" in hpp


def test_cpp_mirror_method_compiles(tmp_path):
    import subprocess
    src = tmp_path / "map.cpp"
    src.write_text('#include <string>\n#include <vector>\n#include "awry.hpp"\n'
                   "uint64_t use(awry::FmIndex& ix) {\n"
                   '  std::vector<std::string> qs{"ACGTACGTACGT", "GATTACAGATTACA"};\n'
                   "  uint64_t s = 0;\n"
                   "  std::vector<uint8_t> status;\n"
                   "  awry::FmIndex::ChainParams p;\n"
                   "  for (auto& per : ix.parallel_map(qs, 12, 50, 4, 2, 4, p, &status))\n"
                   "    for (const awry::FmIndex::Mapping& m : per)\n"
                   "      s += m.pos.seq_idx + m.pos.local_pos + m.t_begin + m.t_end + m.edits + m.chain_score + m.chain_index + m.strand + m.mapq +\n"
                   "           (m.flags & AWRY_MAP_SECONDARY) + m.cigar.size() + m.cigar_string().size();\n"
                   "  static_assert(sizeof(awry_map_t) == 32 && AWRY_MAP_MAX_CHAINS == 8, \"layout\");\n"
                   "  return s + ix.parallel_map(qs).size();\n}\n")
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"), str(src)])


# ---- errors that need no device ------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def hostonly_index():
    t, st, hd = synth.make_text(2_000, 0, 61, 1, 0.0)
    return FmIndex.from_text(t, 0, 8, 0, st, hd, build_device=BUILD_HOST)  # no set_devices: no replica


def test_without_replicas_the_calls_return_no_device(hostonly_index):
    qb, qo = pack_queries([b"ACGTACGTACGT", b"GATTACA"])
    for call in (lambda: hostonly_index.parallel_map_csr(qb, qo), lambda: hostonly_index.parallel_map([b"ACGT"], min_len=1, max_hits=5),
                 lambda: hostonly_index.map_string(b"ACGT"), lambda: hostonly_index.dev_revcomp(None, None, 0, None, None),
                 lambda: hostonly_index.dev_map_select(None, None, None, None, 0, 4, 1, None)):
        with pytest.raises(AwryError) as e:
            call()
        assert e.value.code == ERR_NO_DEVICE


def test_bad_parameters_are_argument_errors(hostonly_index):
    qb, qo = pack_queries([b"ACGTACGTACGT"])
    ix = hostonly_index
    bad = [lambda: ix.parallel_map_csr(qb, qo, chains_per_strand=0), lambda: ix.parallel_map_csr(qb, qo, chains_per_strand=9),
           lambda: ix.parallel_map_csr(qb, qo, max_report=0), lambda: ix.parallel_map_csr(qb, qo, chains_per_strand=3, max_report=7),
           lambda: ix.parallel_map_csr(qb, qo, band=9), lambda: ix.parallel_map_csr(qb, qo, min_len=0), lambda: ix.parallel_map_csr(qb, qo, max_hits=0),
           lambda: ix.parallel_map_csr(qb, qo, lookback=65), lambda: ix.dev_map_select(None, None, None, None, 0, 0, 1, None),
           lambda: ix.dev_map_select(None, None, None, None, 0, 9, 1, None), lambda: ix.dev_map_select(None, None, None, None, 0, 2, 0, None),
           lambda: ix.dev_map_select(None, None, None, None, 0, 2, 5, None)]
    for k, call in enumerate(bad):
        with pytest.raises(AwryError) as e:
            call()
        assert e.value.code == ERR_ARG, k
    # an amino index is an argument error, before any device is asked for
    t, st, hd = synth.make_text(1_000, 1, 5, 1, 0.0)
    aa = FmIndex.from_text(t, 1, 8, 0, st, hd, build_device=BUILD_HOST)
    for call in (lambda: aa.parallel_map_csr(*pack_queries([b"ACDEFGHIKLMN"])), lambda: aa.dev_revcomp(None, None, 0, None, None)):
        with pytest.raises(AwryError) as e:
            call()
        assert e.value.code == ERR_ARG
    aa.close()
    # the out-pointers of a failed call stay as they were; cigar_off_out without cigar_out is an argument error too
    L = _lib.load_library()
    u64p, u8p, u32p = C.POINTER(C.c_uint64), C.POINTER(C.c_uint8), C.POINTER(C.c_uint32)
    for tail in ((0, 1, 4), (9, 1, 4), (4, 0, 4), (4, 9, 4), (4, 1, 9)):
        off, m, ps, coff, cg, st = u64p(), C.POINTER(_lib.Map)(), C.POINTER(_lib.Pos)(), u64p(), u32p(), u8p()
        rc = L.awry_map_batch(ix._h, qb.ctypes.data, qo.ctypes.data_as(u64p), 1, 12, 50, 100, 16, 100, 0, 1, *tail, C.byref(off), C.byref(m), C.byref(ps),
                              C.byref(coff), C.byref(cg), C.byref(st))
        assert rc == ERR_ARG and not off and not m and not ps and not coff and not cg and not st, tail
    off, coff = u64p(), u64p()
    rc = L.awry_map_batch(ix._h, qb.ctypes.data, qo.ctypes.data_as(u64p), 1, 12, 50, 100, 16, 100, 0, 1, 4, 1, 4, C.byref(off), None, None, C.byref(coff), None,
                          None)
    assert rc == ERR_ARG and not off and not coff


# ---- the fixture, from the reference alone ------------------------------------------------------------------------------------------

class HostWorld:
    """the text of the GPU suites with its oracle index and the SMEMs per query, what tests/test_smems_gpu.py's World holds, without
    the GPU index; the SMEMs come from tests/smem_ref.py's form (b), the oracle's counts -- no string search, so 400 reads take seconds"""

    def __init__(self, oracle, text, st, hd, alphabet):
        self.text, self.st, self.hd, self.alphabet = text, st, hd, alphabet
        self.oi = oracle.OracleIndex.from_text(text, alphabet, 8, 0, st, hd)
        self.ctext = ar.canonical_text(text, alphabet)
        self._ref = {}

    def ref(self, q):
        key = bytes(q)
        if key not in self._ref:
            self._ref[key] = sr.smems_oracle(self.oi, q, self.alphabet, 1)
        return self._ref[key]


def fixture_reads(text):
    """the 200 edited reads of the chain-align suite, every second one replaced by its reverse complement
    -> [(read, planted strand, origin of the forward window, planted edit total, indel total)]"""
    return [(mp.rc(q) if i % 2 else q, i % 2, origin, edits, indels) for i, (q, origin, edits, indels) in enumerate(edited_reads(text))]


def placed_count(reads, per_read):
    placed = 0
    for (_, strand, origin, edits, indels), (_, recs, _) in zip(reads, per_read):
        if recs:
            tb, _, e, _, _, s, mapq, flags = recs[0]
            placed += s == strand and e <= edits and abs(tb - origin) <= indels and mapq > 0 and flags == 0
    return placed


def test_the_fixture_reads_are_placed_by_the_reference(oracle):
    w = HostWorld(oracle, *synth.make_text(40_000, 0, 21, 5, 0.03), 0)
    reads = fixture_reads(w.text)
    assert len(reads) == 200 and sum(r[1] for r in reads) == 100
    tsym = [int(v) for v in mr.to_symbols(bytes(w.text), 0)][:-1]
    per = mp.map_reads(tsym, [r[0] for r in reads], lambda qs: want_chains(w, qs, *KEY, E2E_PARAMS[KEY])[0], 4, 1, 4)
    placed = placed_count(reads, per)
    print("fixture reads whose primary has the planted strand, is within the planted edits, at the origin and has MAPQ > 0: %d of %d" % (placed, len(reads)))
    assert placed >= FIXTURE["placed_min"] and placed == FIXTURE["placed"]
