"""Mapping read pairs without a GPU: the pair choice of tests/pair_ref.py on hand-made lists (proper against improper, every tie,
the insert bounds, redundancy of rescued candidates, MAPQ, the single-end cases), the window arithmetic, the C ABI, ctypes, the C++
mirror and the Rust crates agree, the argument errors that need no device come back as status codes, and the character of the
fixture pairs from the reference alone."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from awry_amd import _lib
from awry_amd.fm_index import (BUILD_HOST, ERR_ARG, ERR_NO_DEVICE, MAP_MATE_UNMAPPED, MAP_PROPER_PAIR, MAP_RESCUED, PAIR_MAX_ANCHORS, PAIR_MAX_INSERT,
                               PAIR_NO_CHAIN, AwryError, FmIndex, pack_queries)
from tests import edit_ref as er
from tests import map_ref as mp
from tests import mismatch_ref as mr
from tests import pair_ref as pr
from tests import synth
from tests.test_chain_align_gpu import KEY
from tests.test_chain_gpu import E2E_PARAMS, want_chains
from tests.test_map_cpu import HostWorld

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("awry_map_pairs_batch", "awry_dev_pair_windows", "awry_dev_pair_select")
# what tests/pair_ref.py gives (computed on the CPU when the test was written) for the 200 fixture pairs at (min_len, max_hits) = (12,
# 20), A = 4, band 4 and PAIR_ARGS: the pairs that come out proper with both mates on their planted strands and within their indel
# totals of their origins (the condition is 180), and the mates that are rescued (the condition is 10; 25 are built to seed nowhere)
FIXTURE = dict(proper_min=180, proper=195, rescued_min=10, rescued=25)
PAIR_ARGS = dict(mn=0, mx=1000, U=4, G=2, k=8)

ST, N_TEXT = [0, 10_000, 20_000], 30_000  # the record starts and text length of the hand-made lists
HAND = dict(mn=100, mx=500, U=4, G=2)
NC = PAIR_NO_CHAIN


def c(s, j, e, sc, tb, te):
    return (s, j, e, sc, tb, te)


def z(s, e, tb, te):
    """a rescued record"""
    return (tb, te, e, 0, NC, s, 0, MAP_RESCUED)


def hand_made_pairs():
    """-> [(name, candidates of mate 0, of mate 1, capped 0, capped 1, {(t, a): rescued record}, (sel of mate 0's record, of mate 1's,
    proper, MAPQ, insert))] at HAND's parameters on records [0, 10000), [10000, 20000), [20000, 30000); sel = ("c", index in the kept
    list), ("r", anchor index) or None"""
    x0 = c(0, 0, 1, 80, 1000, 1101)
    out = [
        ("proper beats improper at equal edits", [x0], [c(1, 0, 1, 90, 5000, 5101), c(1, 1, 1, 80, 1300, 1401)], 0, 0, {}, (("c", 0), ("c", 1), True, 40, 401)),
        ("improper wins when it is more than U edits better", [c(0, 0, 0, 80, 1000, 1101)], [c(1, 0, 0, 80, 5000, 5101), c(1, 1, 5, 80, 1300, 1401)], 0, 0, {},
         (("c", 0), ("c", 0), False, 10, 0)),
        ("a tie on cost goes to the proper pair", [c(0, 0, 0, 80, 1000, 1101)], [c(1, 0, 0, 80, 5000, 5101), c(1, 1, 4, 80, 1300, 1401)], 0, 0, {},
         (("c", 0), ("c", 1), True, 0, 401)),
        ("a tie between proper pairs: the smaller index of x", [x0, c(0, 1, 1, 80, 1200, 1301)], [c(1, 0, 1, 80, 1390, 1491)], 0, 0, {},
         (("c", 0), ("c", 0), True, 0, 491)),
        ("then the smaller index of y", [x0], [c(1, 0, 1, 80, 1300, 1401), c(1, 1, 1, 80, 1402, 1499)], 0, 0, {}, (("c", 0), ("c", 0), True, 0, 401)),
        ("the same strand is never proper", [c(0, 0, 0, 80, 1000, 1101)], [c(0, 0, 0, 80, 1300, 1401)], 0, 0, {}, (("c", 0), ("c", 0), False, 60, 0)),
        ("different records are never proper", [c(0, 0, 0, 80, 9800, 9901)], [c(1, 0, 0, 80, 10050, 10151)], 0, 0, {}, (("c", 0), ("c", 0), False, 60, 0)),
        ("f after v is not proper", [c(0, 0, 0, 80, 1300, 1401)], [c(1, 0, 0, 80, 1000, 1101)], 0, 0, {}, (("c", 0), ("c", 0), False, 60, 0)),
        ("f ending after v is not proper", [c(0, 0, 0, 80, 1000, 1201)], [c(1, 0, 0, 80, 1050, 1151)], 0, 0, {}, (("c", 0), ("c", 0), False, 60, 0)),
        ("mate 0 on the reverse strand", [c(1, 0, 0, 80, 1300, 1401)], [c(0, 0, 0, 80, 1000, 1101)], 0, 0, {}, (("c", 0), ("c", 0), True, 60, 401)),
        ("insert exactly at min", [c(0, 0, 0, 80, 1000, 1040)], [c(1, 0, 0, 80, 1050, 1100)], 0, 0, {}, (("c", 0), ("c", 0), True, 60, 100)),
        ("insert one below min", [c(0, 0, 0, 80, 1000, 1040)], [c(1, 0, 0, 80, 1049, 1099)], 0, 0, {}, (("c", 0), ("c", 0), False, 60, 0)),
        ("insert exactly at max", [c(0, 0, 0, 80, 1000, 1101)], [c(1, 0, 0, 80, 1399, 1500)], 0, 0, {}, (("c", 0), ("c", 0), True, 60, 500)),
        ("insert one above max", [c(0, 0, 0, 80, 1000, 1101)], [c(1, 0, 0, 80, 1400, 1501)], 0, 0, {}, (("c", 0), ("c", 0), False, 60, 0)),
        ("empty spans", [c(0, 0, 0, 80, 1000, 1000)], [c(1, 0, 0, 80, 1200, 1200)], 0, 0, {}, (("c", 0), ("c", 0), True, 60, 200)),
        ("a rescued candidate dropped against an original, another kept and chosen", [c(0, 0, 2, 80, 1000, 1101)], [c(1, 0, 2, 80, 5000, 5101)], 0, 0,
         {(1, 0): z(1, 0, 5050, 5151), (0, 0): z(0, 3, 4700, 4801)}, (("r", 0), ("c", 0), True, 30, 401)),
        ("a rescued candidate dropped against an earlier rescued one", [c(0, 0, 2, 80, 1000, 1101), c(0, 1, 2, 70, 7000, 7101)], [], 0, 0,
         {(1, 0): z(1, 1, 1300, 1401), (1, 1): z(1, 0, 1350, 1451)}, (("c", 0), ("r", 0), True, 40, 401)),
        ("an empty rescued span intersects nothing, the other strand neither", [c(0, 0, 2, 80, 1000, 1101)], [c(1, 0, 3, 80, 1300, 1401)], 0, 0,
         {(1, 0): z(1, 1, 1350, 1350), (1, 1): z(0, 0, 1300, 1401)}, (("c", 0), ("r", 0), True, 20, 350)),
        ("no rescue hit in any slot", [x0], [], 0, 0, {(1, 0): None, (1, 1): None}, (("c", 0), None, False, 60, 0)),
        ("a proper pair alone has MAPQ 60", [x0], [c(1, 0, 1, 80, 1300, 1401)], 0, 0, {}, (("c", 0), ("c", 0), True, 60, 401)),
        ("a capped read has pair MAPQ 0", [x0], [c(1, 0, 1, 80, 1300, 1401)], 1, 0, {}, (("c", 0), ("c", 0), True, 0, 401)),
        ("the mate capped", [x0], [c(1, 0, 1, 80, 1300, 1401)], 0, 1, {}, (("c", 0), ("c", 0), True, 0, 401)),
        ("one list empty: the single-end primary and its MAPQ", [c(0, 1, 3, 80, 7000, 7101), x0], [], 0, 0, {}, (("c", 0), None, False, 20, 0)),
        ("the other list empty, capped", [], [c(1, 0, 1, 80, 1300, 1401)], 0, 1, {}, (None, ("c", 0), False, 0, 0)),
        ("both lists empty", [], [], 0, 0, {}, (None, None, False, None, 0)),
    ]
    out += [("cost2 - cost1 = %d" % d, [c(0, 0, 0, 80, 1000, 1101)], [c(1, 0, 0, 80, 1300, 1401), c(1, 1, d, 70, 1200, 1290)], 0, 0, {},
             (("c", 0), ("c", 0), True, q, 401)) for d, q in ((0, 0), (1, 10), (5, 50), (6, 60), (7, 60))]
    return out


def run_hand(case):
    _, c0, c1, cap0, cap1, resc, _ = case
    return pr.rank_pairs(c0, c1, bool(cap0), bool(cap1), resc, ST, HAND["mn"], HAND["mx"], HAND["U"])


def test_pair_choice_on_hand_made_lists():
    cases = hand_made_pairs()
    assert len({case[0] for case in cases}) == len(cases) == 30
    for case in cases:
        name, c0, c1, cap0, cap1, resc, (sel0, sel1, proper, mapq, insert) = case
        recs, ins, sel = run_hand(case)
        assert sel == [sel0, sel1] and ins == insert, (name, recs, ins, sel)
        K = [pr.kept_list(c0, bool(cap0)), pr.kept_list(c1, bool(cap1))]
        for m, (r, s) in enumerate(zip(recs, sel)):
            assert (r is None) == (s is None), name
            if r is None:
                continue
            src = K[m][s[1]] if s[0] == "c" else resc[(m, s[1])]
            assert r[:6] == src[:6], (name, m)
            if sel0 is not None and sel1 is not None:
                assert r[6] == mapq and r[7] == (MAP_PROPER_PAIR if proper else 0) | (MAP_RESCUED if s[0] == "r" else 0), (name, m, r)
            else:  # the single-end primary, exactly as the single-end ranking reports it
                assert r == mp.rank_candidates([c0, c1][m], bool([cap0, cap1][m]), 1)[0][0][:7] + (MAP_MATE_UNMAPPED,) and r[6] == mapq, (name, m, r)
        # the input order of the lists changes nothing: the rank is a total order
        assert pr.rank_pairs(c0[::-1], c1[::-1], bool(cap0), bool(cap1), resc, ST, HAND["mn"], HAND["mx"], HAND["U"]) == (recs, ins, sel), name
    # a larger penalty turns the improper winner into the loser; U = 0 makes the orders of cost alone
    _, c0, c1, *_ = cases[1]
    assert pr.rank_pairs(c0, c1, False, False, {}, ST, 100, 500, 6)[2] == [("c", 0), ("c", 1)]
    assert pr.rank_pairs(c0, c1, False, False, {}, ST, 100, 500, 0)[0][0][6:] == (50, 0)
    # proper() itself, on records
    f, v = (1000, 1101, 0, 80, 0, 0, 0, 0), (1300, 1401, 0, 80, 0, 1, 0, 0)
    assert pr.proper(f, v, ST, 100, 500) and pr.proper(v, f, ST, 100, 500) and not pr.proper(f, f, ST, 100, 500) and pr.insert_of(v, f) == 401
    assert not pr.proper(f, v, ST, 402, 500) and not pr.proper(f, v, ST, 100, 400) and pr.proper(f, v, ST, 401, 401)


def test_windows_of_on_hand_made_lists():
    rec = lambda s, tb, te: (tb, te, 0, 80, 0, s, 60, 0)
    W = lambda K0, K1, L0=101, L1=101, mn=100, mx=500, G=2, k=4, p=0: pr.windows_of(K0, K1, L0, L1, ST, N_TEXT, mn, mx, G, k, p)
    none0, none1 = (2, 0, 0), (0, 0, 0)  # what a slot that is no anchor holds: the other mate's strand-0 query, nothing to scan
    # an anchor on the forward strand seeks the reverse strand of its mate downstream; one on the reverse strand the forward strand upstream
    assert W([rec(0, 1000, 1101)], []) == [(3, 1000, 404), none0, none1, none1]
    assert W([rec(1, 1300, 1401)], []) == [(2, 901, 400), none0, none1, none1]
    assert W([], [rec(0, 1000, 1101)], p=3) == [(14, 0, 0), (14, 0, 0), (13, 1000, 404), (12, 0, 0)]
    # min_insert beyond the mate's length and the edits moves the first start
    assert W([rec(0, 1000, 1101)], [], mn=300) == [(3, 1000 + 300 - 101 - 4, 404 - 195), none0, none1, none1]
    # saturation at the text's start, cuts at the record borders and at the text's end
    assert W([rec(1, 200, 301)], [])[0] == (2, 0, 201)
    assert W([rec(0, 9800, 9901)], [])[0] == (3, 9800, 200)
    assert W([rec(1, 10100, 10201)], [])[0] == (2, 10000, 101)
    assert W([rec(0, 29800, 29901)], [])[0] == (3, 29800, 200)
    assert W([rec(0, 9999, 10100)], [])[0] == (3, 9999, 1)  # (the record is t_begin's)
    # the other mate's length: too long for the scan, not longer than k, longer than max_insert + k
    assert W([rec(0, 1000, 1101)], [], L1=257)[0] == none0 and W([rec(0, 1000, 1101)], [], L1=256)[0] == (3, 1000, 500 - 256 + 4 + 1)
    assert W([rec(0, 1000, 1101)], [], L1=4)[0] == none0 and W([rec(0, 1000, 1101)], [], L1=5)[0] == (3, 1091, 409)
    assert W([rec(0, 1000, 1101)], [], mn=0, mx=50)[0] == (3, 0, 0) and W([rec(0, 1000, 1101)], [], mn=0, mx=97)[0] == (3, 1000, 1)
    assert W([rec(1, 1300, 1401)], [], mn=0, mx=50)[0] == (2, 0, 0)  # lo = 1351 > hi = 1300
    # a candidate that is proper with one of the mate's is no anchor; the improper one next to it is
    K0, K1 = [rec(0, 1000, 1101), rec(0, 7000, 7101)], [rec(1, 1300, 1401)]
    assert W(K0, K1) == [none0, (3, 7000, 404), none1, none1]
    # G below, at and above the list's length
    K = [rec(0, 1000, 1101), rec(0, 3000, 3101), rec(1, 5300, 5401)]
    for G in (1, 2, 3, 4):
        got = W(K, [], G=G)
        want = [(3, 1000, 404), (3, 3000, 404), (2, 4901, 400), none0][:G]
        assert len(got) == 2 * G and got[:G] == want[:G] and got[G:] == [none1] * G, G
    assert W(K, [], G=0) == []


# ---- declarations ---------------------------------------------------------------------------------------------------------------------

def test_header_ctypes_cpp_mirror_and_rust_agree():
    L = _lib.load_library()
    for name in ENTRY_POINTS:
        assert name in _lib.header_symbols(), name
        assert getattr(L, name) is not None, name
    header = open(os.path.join(ROOT, "include", "awry_hip.h")).read()
    for word in ("AWRY_PAIR_MAX_INSERT = 1 << 20", "AWRY_PAIR_MAX_ANCHORS = 4", "AWRY_MAP_PROPER_PAIR = 2", "AWRY_MAP_RESCUED = 4", "AWRY_MAP_MATE_UNMAPPED = 8",
                 "#define AWRY_PAIR_NO_CHAIN 0xFFFFFFFFu", "map read pairs: insert-size pairing, mate rescue, proper-pair flag"):
        assert word in header, word
    assert header.index("map reads on both strands") < header.index("map read pairs: insert-size pairing") < header.index("releases an array one of the calls above")
    assert (MAP_PROPER_PAIR, MAP_RESCUED, MAP_MATE_UNMAPPED) == (2, 4, 8) == (pr.MAP_PROPER_PAIR, pr.MAP_RESCUED, pr.MAP_MATE_UNMAPPED)
    assert (PAIR_MAX_INSERT, PAIR_MAX_ANCHORS, PAIR_NO_CHAIN) == (1 << 20, 4, 0xFFFFFFFF) == (pr.PAIR_MAX_INSERT, pr.PAIR_MAX_ANCHORS, pr.PAIR_NO_CHAIN)
    src = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in ENTRY_POINTS:
        args = re.search(r"\b%s\s*\(([^)]*)\)" % name, src).group(1)
        assert len(args.split(",")) == len(getattr(L, name).argtypes), name
    rust = open(os.path.join(ROOT, "rust", "awry-hip-sys", "src", "lib.rs")).read()
    for word in ("pub const AWRY_MAP_PROPER_PAIR: u16 = 2;", "pub const AWRY_MAP_RESCUED: u16 = 4;", "pub const AWRY_MAP_MATE_UNMAPPED: u16 = 8;",
                 "pub const AWRY_PAIR_MAX_INSERT: u64 = 1 << 20;", "pub const AWRY_PAIR_MAX_ANCHORS: u32 = 4;", "pub const AWRY_PAIR_NO_CHAIN: u32 = 0xFFFF_FFFF;",
                 "pub fn awry_map_pairs_batch(", "pub fn awry_dev_pair_windows(", "pub fn awry_dev_pair_select("):
        assert word in rust, word
    safe = open(os.path.join(ROOT, "rust", "awry", "src", "fm_index.rs")).read()
    assert "pub fn parallel_map_pairs(" in safe and "sys::awry_map_pairs_batch(" in safe and "pub struct PairParams {" in safe
    assert "PairParams { min_insert: 0, max_insert: 1000, unpaired_penalty: 4, rescue_anchors: 2, rescue_edits: 4 }" in safe
    hpp = open(os.path.join(ROOT, "include", "awry.hpp")).read()
    assert "parallel_map_pairs(" in hpp and "awry_map_pairs_batch(" in hpp
    import inspect
    sig = inspect.signature(FmIndex.parallel_map_pairs_csr).parameters
    assert [sig[k].default for k in ("min_insert", "max_insert", "unpaired_penalty", "rescue_anchors", "rescue_edits")] == [0, 1000, 4, 2, 4]
    sig = inspect.signature(FmIndex.parallel_map_pairs).parameters
    assert [sig[k].default for k in ("min_insert", "max_insert", "unpaired_penalty", "rescue_anchors", "rescue_edits")] == [0, 1000, 4, 2, 4]


def test_cpp_mirror_method_compiles(tmp_path):
    src = tmp_path / "pairs.cpp"
    src.write_text('#include <string>\n#include <vector>\n#include "awry.hpp"\n'
                   "uint64_t use(awry::FmIndex& ix) {\n"
                   '  std::vector<std::string> r1{"ACGTACGTACGT", "GATTACAGATTACA"}, r2{"TTTTACGTACGT", "GATTACAGACCACA"};\n'
                   "  uint64_t s = 0;\n"
                   "  std::vector<uint8_t> status;\n"
                   "  awry::FmIndex::PairParams pp;\n"
                   "  pp.max_insert = 600; pp.rescue_edits = 8;\n"
                   "  for (const awry::FmIndex::PairMapping& pm : ix.parallel_map_pairs(r1, r2, 12, 50, 4, 4, pp, awry::FmIndex::ChainParams(), &status)) {\n"
                   "    s += pm.insert;\n"
                   "    for (const awry::FmIndex::Mapping& m : pm.mate1) s += m.t_begin + (m.flags & AWRY_MAP_PROPER_PAIR) + (m.flags & AWRY_MAP_RESCUED);\n"
                   "    for (const awry::FmIndex::Mapping& m : pm.mate2) s += m.t_end + (m.flags & AWRY_MAP_MATE_UNMAPPED) + (m.chain_index == AWRY_PAIR_NO_CHAIN);\n"
                   "  }\n"
                   "  static_assert(AWRY_PAIR_MAX_INSERT == 1 << 20 && AWRY_PAIR_MAX_ANCHORS == 4, \"limits\");\n"
                   "  return s + ix.parallel_map_pairs(r1, r2).size();\n}\n")
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"), str(src)])


# ---- errors that need no device ------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def hostonly_index():
    t, st, hd = synth.make_text(2_000, 0, 61, 1, 0.0)
    return FmIndex.from_text(t, 0, 8, 0, st, hd, build_device=BUILD_HOST)  # no set_devices: no replica


def test_without_replicas_the_calls_return_no_device(hostonly_index):
    qb, qo = pack_queries([b"ACGTACGTACGT", b"GATTACA"])
    for call in (lambda: hostonly_index.parallel_map_pairs_csr(qb, qo), lambda: hostonly_index.parallel_map_pairs([b"ACGT"], [b"ACGG"], min_len=1, max_hits=5),
                 lambda: hostonly_index.dev_pair_windows(None, None, None, 0, 0, 1000, 2, 4, None, None, None),
                 lambda: hostonly_index.dev_pair_select(None, None, None, None, 0, 0, 1000, 4, 2, None)):
        with pytest.raises(AwryError) as e:
            call()
        assert e.value.code == ERR_NO_DEVICE


def test_bad_parameters_are_argument_errors(hostonly_index):
    qb, qo = pack_queries([b"ACGTACGTACGT", b"GATTACAGATTACA"])
    qb3, qo3 = pack_queries([b"ACGTACGTACGT", b"GATTACAGATTACA", b"ACGTACGTACGT"])
    ix = hostonly_index
    bad = [lambda: ix.parallel_map_pairs_csr(qb3, qo3),  # an odd number of reads
           lambda: ix.parallel_map_pairs_csr(qb, qo, min_insert=501, max_insert=500), lambda: ix.parallel_map_pairs_csr(qb, qo, max_insert=PAIR_MAX_INSERT + 1),
           lambda: ix.parallel_map_pairs_csr(qb, qo, unpaired_penalty=256), lambda: ix.parallel_map_pairs_csr(qb, qo, rescue_anchors=5),
           lambda: ix.parallel_map_pairs_csr(qb, qo, rescue_edits=9), lambda: ix.parallel_map_pairs_csr(qb, qo, rescue_edits=-1),
           lambda: ix.parallel_map_pairs_csr(qb, qo, chains_per_strand=0), lambda: ix.parallel_map_pairs_csr(qb, qo, chains_per_strand=9),
           lambda: ix.parallel_map_pairs_csr(qb, qo, band=9), lambda: ix.parallel_map_pairs_csr(qb, qo, min_len=0), lambda: ix.parallel_map_pairs_csr(qb, qo, max_hits=0),
           lambda: ix.dev_pair_windows(None, None, None, 0, 2, 1, 2, 4, None, None, None), lambda: ix.dev_pair_windows(None, None, None, 0, 0, 1000, 5, 4, None, None, None),
           lambda: ix.dev_pair_windows(None, None, None, 0, 0, 1000, 2, 9, None, None, None),
           lambda: ix.dev_pair_select(None, None, None, None, 0, 0, PAIR_MAX_INSERT + 1, 4, 2, None),
           lambda: ix.dev_pair_select(None, None, None, None, 0, 0, 1000, 256, 2, None), lambda: ix.dev_pair_select(None, None, None, None, 0, 0, 1000, 4, 5, None)]
    for k, call in enumerate(bad):
        with pytest.raises(AwryError) as e:
            call()
        assert e.value.code == ERR_ARG, k
    # the limits themselves pass the argument checks: what is left to fail is the missing replica
    for call in (lambda: ix.parallel_map_pairs_csr(qb, qo, min_insert=PAIR_MAX_INSERT, max_insert=PAIR_MAX_INSERT, unpaired_penalty=255, rescue_anchors=4, rescue_edits=8),
                 lambda: ix.parallel_map_pairs_csr(qb, qo, unpaired_penalty=0, rescue_anchors=0, rescue_edits=0)):
        with pytest.raises(AwryError) as e:
            call()
        assert e.value.code == ERR_NO_DEVICE
    # an amino index is an argument error, before any device is asked for
    t, st, hd = synth.make_text(1_000, 1, 5, 1, 0.0)
    aa = FmIndex.from_text(t, 1, 8, 0, st, hd, build_device=BUILD_HOST)
    for call in (lambda: aa.parallel_map_pairs_csr(*pack_queries([b"ACDEFGHIKLMN", b"ACDEFGHIKLMN"])),
                 lambda: aa.dev_pair_windows(None, None, None, 0, 0, 1000, 2, 4, None, None, None),
                 lambda: aa.dev_pair_select(None, None, None, None, 0, 0, 1000, 4, 2, None)):
        with pytest.raises(AwryError) as e:
            call()
        assert e.value.code == ERR_ARG
    aa.close()
    # the out-pointers of a failed call stay as they were; cigar_off_out without cigar_out is an argument error too
    L = _lib.load_library()
    u64p, u8p, u32p = C.POINTER(C.c_uint64), C.POINTER(C.c_uint8), C.POINTER(C.c_uint32)
    for n, tail in ((3, (4, 4, 0, 1000, 4, 2, 4)), (2, (4, 4, 2, 1, 4, 2, 4)), (2, (4, 4, 0, PAIR_MAX_INSERT + 1, 4, 2, 4)), (2, (4, 4, 0, 1000, 256, 2, 4)),
                    (2, (4, 4, 0, 1000, 4, 5, 4)), (2, (4, 4, 0, 1000, 4, 2, 9))):
        off, m, ps, coff, cg, st, ins = u64p(), C.POINTER(_lib.Map)(), C.POINTER(_lib.Pos)(), u64p(), u32p(), u8p(), u32p()
        rc = L.awry_map_pairs_batch(ix._h, qb3.ctypes.data, qo3.ctypes.data_as(u64p), n, 12, 50, 100, 16, 100, 0, 1, *tail, C.byref(off), C.byref(m),
                                    C.byref(ps), C.byref(coff), C.byref(cg), C.byref(st), C.byref(ins))
        assert rc == ERR_ARG and not off and not m and not ps and not coff and not cg and not st and not ins, tail
    off, coff = u64p(), u64p()
    rc = L.awry_map_pairs_batch(ix._h, qb.ctypes.data, qo.ctypes.data_as(u64p), 2, 12, 50, 100, 16, 100, 0, 1, 4, 4, 0, 1000, 4, 2, 4, C.byref(off), None, None,
                                C.byref(coff), None, None, None)
    assert rc == ERR_ARG and not off and not coff


# ---- the fixture, from the reference alone ------------------------------------------------------------------------------------------

def unseedable(q):
    """96 letters with a substitution every 11th letter: no exact run reaches min_len = 12, and that is 8 edits"""
    q = bytearray(q[:96])
    for at in range(10, 96, 11):
        q[at] = b"ACGT"[(b"ACGT".index(q[at]) + 1) % 4]
    return bytes(q)


def fixture_pairs(text, st, n=200, seed=71):
    """n simulated pairs: fragments of 150..600 letters inside one record and free of N, mates of 101 letters from the fragment's two
    ends with 0..2 substitutions and at most one indel of one letter each, every second pair taken from the reverse strand (mate 0 is
    the fragment's right end); in every eighth pair one mate -- mate 0 and mate 1 in turn -- is `unseedable`
    -> [(mate 0, mate 1, (strand, origin, indel total) of mate 0, the same of mate 1)]; origin: where the mate's forward window begins"""
    rng = np.random.default_rng(seed)
    body, bounds = bytes(text[:-1]), [int(x) for x in st] + [len(text) - 1]
    out = []
    while len(out) < n:
        F, r = int(rng.integers(150, 601)), int(rng.integers(0, len(st)))
        at = int(rng.integers(bounds[r], bounds[r + 1] - F))
        frag = body[at:at + F]
        if any(ch not in b"ACGT" for ch in frag):
            continue
        i = len(out)
        hard = (i // 8) % 2 if i % 8 == 3 else None  # which mate seeds nowhere
        mates = []
        for m, (w, origin) in enumerate(((frag[:101], at), (frag[-101:], at + F - 101))):
            if hard == m:  # (of the right end the last 96 letters, so that the fragment's outer end stays)
                mates.append((unseedable(frag[:96]), at, 0) if m == 0 else (unseedable(frag[-96:]), at + F - 96, 0))
                continue
            q, indels = bytearray(w), 0
            for _ in range(int(rng.integers(0, 3))):
                p = int(rng.integers(0, len(q)))
                q[p] = b"ACGT"[(b"ACGT".index(q[p]) + 1 + int(rng.integers(0, 3))) % 4]
            if rng.random() < 0.3:
                p = int(rng.integers(30, 70))
                if rng.random() < 0.5:
                    del q[p]
                else:
                    q[p:p] = b"ACGT"[int(rng.integers(0, 4)):][:1]
                indels = 1
            mates.append((bytes(q), origin, indels))
        (f, fo, fi), (v, vo, vi) = mates
        fwd, rev = (f, (0, fo, fi)), (mp.rc(v), (1, vo, vi))
        a, b = (rev, fwd) if i % 2 else (fwd, rev)
        out.append((a[0], b[0], a[1], b[1]))
    return out


def fixture_character(pairs, per_read):
    """-> (pairs that come out proper with both mates on their planted strands within their indel totals of their origins, rescued mates)"""
    good = rescued = 0
    for p, (_, _, w0, w1) in enumerate(pairs):
        recs = [per_read[2 * p + m][1] for m in (0, 1)]
        rescued += sum(1 for r in recs if r and r[0][7] & MAP_RESCUED)
        good += all(r and r[0][7] & MAP_PROPER_PAIR and r[0][5] == w[0] and abs(r[0][0] - w[1]) <= w[2] for r, w in zip(recs, (w0, w1)))
    return good, rescued


def interleaved(pairs):
    return [q for p in pairs for q in p[:2]]


def test_the_fixture_pairs_are_paired_and_rescued_by_the_reference(oracle):
    w = HostWorld(oracle, *synth.make_text(40_000, 0, 21, 5, 0.03), 0)
    pairs = fixture_pairs(w.text, w.st)
    assert len(pairs) == 200 and sum(p[2][0] for p in pairs) == 100 and all(len(p[0]) in (96, 100, 101, 102) for p in pairs)
    hard = [q for p in pairs for q in p[:2] if len(q) == 96]
    assert len(hard) == 25 >= 20
    chains_of = lambda qs: want_chains(w, qs, *KEY, E2E_PARAMS[KEY])[0]
    assert all(not ch for q in hard for _, ch in chains_of(mp.doubled([q])))  # built to seed nowhere: no SMEM of 12 letters, no chain
    t = er.Text(w.text, 0)
    tsym = [int(v) for v in mr.to_symbols(bytes(w.text), 0)][:-1]
    a = PAIR_ARGS
    per, inserts = pr.map_pairs(t, tsym, interleaved(pairs), chains_of, 4, 4, w.st, a["mn"], a["mx"], a["U"], a["G"], a["k"])
    good, rescued = fixture_character(pairs, per)
    print("fixture pairs that come out proper with both mates at their origins: %d of %d; rescued mates: %d" % (good, len(pairs), rescued))
    assert good >= FIXTURE["proper_min"] and rescued >= FIXTURE["rescued_min"]
    assert (good, rescued) == (FIXTURE["proper"], FIXTURE["rescued"])
    assert sum(1 for x in inserts if x) >= good and all(150 - 2 <= x <= 600 + 2 for x in inserts if x)
