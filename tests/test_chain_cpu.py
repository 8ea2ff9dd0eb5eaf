"""Chaining without a GPU: the two forms of tests/chain_ref.py agree with each other on random seed sets, the properties the header
states hold, the C ABI, ctypes, the C++ mirror and the Rust sys crate agree, and the argument / no-replica errors come back as
status codes."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from awry_amd import _lib
from awry_amd.fm_index import (BUILD_HOST, CHAIN_DTYPE, CHAIN_MAX_LOOKBACK, CHAIN_MAX_SEEDS, ERR_ARG, ERR_NO_DEVICE, Q_SEED_CAP, SEED_DTYPE, AwryError,
                               FmIndex, pack_queries)
from tests import chain_ref as cr
from tests import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("awry_chain_batch", "awry_dev_chain_seeds", "awry_dev_chain_seeds_tally")
STARTS = [0, 700, 1500]  # record starts of the random sets: joins inside the coordinate range


def random_seed_set(rng, n):
    """n seeds; small coordinate ranges force ties in every key and equal scores"""
    span = int(rng.choice([4, 12, 60, 400, 2500]))
    lens = (1, 2, 3, 5, 19) if rng.random() < 0.7 else (7,)
    return [(int(rng.integers(0, span)), int(rng.choice(lens)), int(rng.integers(0, span))) for _ in range(n)]


def random_params(rng):
    return cr.Params(int(rng.choice([5, 50, 4096])), int(rng.choice([1, 2, 3, 16, 17, 64])), int(rng.choice([1, 3, 30, 5000])),
                     int(rng.choice([0, 1, 5, 1000])), int(rng.choice([1, 2, 10])))


@pytest.fixture(scope="module")
def random_cases():
    rng = np.random.default_rng(2024)
    sizes = list(range(0, 201)) + [int(rng.integers(0, 40)) for _ in range(1799)]
    return [(random_seed_set(rng, n), random_params(rng)) for n in sizes]


def test_the_two_forms_agree_on_2000_random_seed_sets(random_cases):
    assert len(random_cases) == 2000 and {len(s) for s, _ in random_cases} >= set(range(201))
    multi = truncated = tied = capped = 0
    for seeds, P in random_cases:
        st, chains, tally = cr.chain_query(seeds, STARTS, P)
        assert (st, chains) == cr.chain_query_full(seeds, STARTS, P), (seeds, P)
        capped += st == Q_SEED_CAP
        assert (st == Q_SEED_CAP) == (len(seeds) > P.max_seeds) and (st == 0 or not chains)
        multi += any(c[1] > 1 for c in chains)
        tied += len({(s[2], s[0]) for s in seeds}) < len(seeds)
        if st == 0:
            truncated += any(b > 0 for b in cr.chain_bases(seeds, STARTS, P))
            assert tally == (len(seeds), sum(min(i, P.lookback) for i in range(len(seeds))), len(chains))
    assert multi > 300 and truncated > 50 and tied > 500 and capped > 20  # the sets do chain, truncate, tie and hit the cap


def test_a_window_that_holds_every_seed_equals_the_unwindowed_programme(random_cases):
    differs = 0
    for seeds, P in random_cases[:600]:
        if len(seeds) > P.max_seeds:
            continue
        wide = P._replace(lookback=max(1, len(seeds)))
        s = cr.sort_seeds(seeds)
        rec = [cr.record_of(STARTS, x[2]) for x in s]
        f, p, _ = cr.scores(s, rec, wide)
        f2, p2 = cr.scores_full(s, rec, P._replace(lookback=10 ** 9))
        assert (f, p) == (f2, p2)
        differs += (f, p) != tuple(cr.scores(s, rec, P)[:2])
    assert differs > 20  # (and the narrow windows of the cases do cut predecessors off)


def test_score_bounds_membership_and_positive_scores(random_cases):
    for seeds, P in random_cases:
        if len(seeds) > P.max_seeds:
            continue
        s = cr.sort_seeds(seeds)
        rec = [cr.record_of(STARTS, x[2]) for x in s]
        f, p, _ = cr.scores(s, rec, P)
        equal_lengths = len({x[1] for x in s}) <= 1
        for i in range(len(s)):
            c = i
            while p[c] is not None:
                assert p[c] < c and c - p[c] <= P.lookback
                c = p[c]
            # the header's consequence: f_i <= q_len_c + (q_begin_i - q_begin_c), c the seed i's predecessors lead back to
            assert s[i][1] <= f[i] <= s[c][1] + s[i][0] - s[c][0]
            if equal_lengths:  # seeds of one length: f_i <= q_begin_i + q_len_i
                assert f[i] <= s[i][0] + s[i][1]
        _, chains, _ = cr.chain_query(seeds, STARTS, P)
        assert all(c[0] >= P.min_score >= 1 and c[1] == len(c[6]) >= 1 for c in chains)
        # every seed belongs to at most one chain: the members, as a multiset, are part of the seeds
        left = sorted(seeds)
        for m in (m for c in chains for m in c[6]):
            left.remove(m)
        for c in chains:
            assert c[6] == cr.sort_seeds(c[6]) and (c[2], c[4]) == (c[6][0][0], c[6][0][2])
            assert c[3] == max(m[0] + m[1] for m in c[6]) and c[5] == max(m[2] + m[1] for m in c[6])
    assert sum(len({x[1] for x in s}) <= 1 and len(s) > 3 for s, _ in random_cases) > 200  # (the one-length bound is exercised)


def test_unequal_lengths_break_the_one_length_bound():
    # what the header's remark says: a long seed followed by a short one that begins inside it
    P = cr.Params(10, 4, 100, 10, 1)
    _, chains, _ = cr.chain_query([(0, 100, 1000), (50, 52, 1049)], [0], P)
    assert chains[0][0] == 100 + min(52, 50, 49) - 1 > 50 + 52


def test_hand_worked_example():
    P = cr.Params(10, 8, 100, 5, 10)
    seeds = [(30, 12, 5030), (0, 20, 5000), (60, 15, 5062), (10, 14, 9000)]
    st, chains, tally = cr.chain_query(seeds, [0], P)
    # sorted by t_pos: (0,20,5000) (30,12,5030) (60,15,5062) (10,14,9000); f = 20, 32, 32 + min(15, 30, 32) - 2 = 45, 14
    assert st == 0 and tally == (4, 6, 2)
    assert chains == [(45, 3, 0, 75, 5000, 5077, [(0, 20, 5000), (30, 12, 5030), (60, 15, 5062)]), (14, 1, 10, 24, 9000, 9014, [(10, 14, 9000)])]


def test_header_ctypes_cpp_mirror_and_rust_agree():
    L = _lib.load_library()
    for name in ENTRY_POINTS:
        assert name in _lib.header_symbols(), name
        assert getattr(L, name) is not None, name
    header = open(os.path.join(ROOT, "include", "awry_hip.h")).read()
    for word in ("AWRY_CHAIN_MAX_SEEDS = 4096", "AWRY_CHAIN_MAX_LOOKBACK = 64", "AWRY_Q_SEED_CAP = 8",
                 "typedef struct { uint32_t q_begin, q_len; uint64_t t_pos; } awry_seed_t;",
                 "typedef struct { uint32_t score, n_seeds, q_begin, q_end; uint64_t t_begin, t_end; } awry_chain_t;"):
        assert word in header, word
    assert (CHAIN_MAX_SEEDS, CHAIN_MAX_LOOKBACK, Q_SEED_CAP) == (4096, 64, 8) == (cr.MAX_SEEDS, cr.MAX_LOOKBACK, cr.Q_SEED_CAP)
    assert C.sizeof(_lib.Seed) == 16 == SEED_DTYPE.itemsize and C.sizeof(_lib.Chain) == 32 == CHAIN_DTYPE.itemsize
    for struct, dtype in ((_lib.Seed, SEED_DTYPE), (_lib.Chain, CHAIN_DTYPE)):
        assert [(n, getattr(struct, n).offset) for n, _ in struct._fields_] == [(n, dtype.fields[n][1]) for n in dtype.names]
    # the argument lists of the header and of ctypes have the same length
    src = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in ENTRY_POINTS:
        args = re.search(r"\b%s\s*\(([^)]*)\)" % name, src).group(1)
        assert len(args.split(",")) == len(getattr(L, name).argtypes), name
    rust = open(os.path.join(ROOT, "rust", "awry-hip-sys", "src", "lib.rs")).read()
    for word in ("pub struct awry_seed_t {\n    pub q_begin: u32,\n    pub q_len: u32,\n    pub t_pos: u64,\n}",
                 "pub struct awry_chain_t {\n    pub score: u32,\n    pub n_seeds: u32,\n    pub q_begin: u32,\n    pub q_end: u32,\n    pub t_begin: u64,\n"
                 "    pub t_end: u64,\n}", "pub fn awry_chain_batch(", "pub fn awry_dev_chain_seeds(", "pub fn awry_dev_chain_seeds_tally("):
        assert word in rust, word
    safe = open(os.path.join(ROOT, "rust", "awry", "src", "fm_index.rs")).read()
    assert "pub fn parallel_chains<'a>(" in safe and "sys::awry_chain_batch(" in safe


@pytest.fixture(scope="module")
def hostonly_index():
    text, st, hd = synth.make_text(2_000, 0, 61, 1, 0.0)
    return FmIndex.from_text(text, 0, 8, 0, st, hd, build_device=BUILD_HOST)  # no set_devices: no replica


def test_without_replicas_the_calls_return_no_device(hostonly_index):
    qb, qo = pack_queries([b"ACGTACGTACGT", b"GATTACA"])
    for call in (lambda: hostonly_index.parallel_chains_csr(qb, qo), lambda: hostonly_index.parallel_chains([b"ACGT"], min_len=1, max_hits=5),
                 lambda: hostonly_index.chains_string(b"ACGT"), lambda: hostonly_index.dev_chain_seeds(None, None, 0, 10, 4, 100, 10, 1, None, None),
                 lambda: hostonly_index.dev_chain_seeds_tally(None, None, 0, 10, 4, 100, 10, 1, None, None, None)):
        with pytest.raises(AwryError) as e:
            call()
        assert e.value.code == ERR_NO_DEVICE


BAD_PARAMS = [dict(max_seeds=0), dict(max_seeds=4097), dict(lookback=0), dict(lookback=65), dict(max_gap=0), dict(min_score=0)]


def test_bad_parameters_are_argument_errors(hostonly_index):
    qb, qo = pack_queries([b"ACGTACGTACGT"])
    good = dict(max_seeds=100, lookback=16, max_gap=100, max_skew=0, min_score=1)
    bad = [lambda kw=kw: hostonly_index.parallel_chains_csr(qb, qo, 12, 50, **dict(good, **kw)) for kw in BAD_PARAMS]
    bad += [lambda: hostonly_index.parallel_chains_csr(qb, qo, 0, 50), lambda: hostonly_index.parallel_chains_csr(qb, qo, 12, 0)]
    for kw in BAD_PARAMS:
        a = dict(good, **kw)
        order = (a["max_seeds"], a["lookback"], a["max_gap"], a["max_skew"], a["min_score"])
        bad.append(lambda o=order: hostonly_index.dev_chain_seeds(None, None, 0, *o, None, None))
        bad.append(lambda o=order: hostonly_index.dev_chain_seeds_tally(None, None, 0, *o, None, None, None))
    for call in bad:
        with pytest.raises(AwryError) as e:
            call()
        assert e.value.code == ERR_ARG
    # the out-pointers of a failed call stay as they were; seed_off_out without seeds_out is an argument error too
    L = _lib.load_library()
    u64p, u8p = C.POINTER(C.c_uint64), C.POINTER(C.c_uint8)
    for args in ((12, 50, 0, 16, 100, 0, 1), (12, 50, 100, 65, 100, 0, 1), (12, 50, 100, 16, 0, 0, 1), (12, 50, 100, 16, 100, 0, 0), (0, 50, 100, 16, 100, 0, 1),
                 (12, 0, 100, 16, 100, 0, 1)):
        off, ch, soff, sd, st = u64p(), C.POINTER(_lib.Chain)(), u64p(), C.POINTER(_lib.Seed)(), u8p()
        rc = L.awry_chain_batch(hostonly_index._h, qb.ctypes.data, qo.ctypes.data_as(u64p), 1, *args, C.byref(off), C.byref(ch), C.byref(soff), C.byref(sd),
                                C.byref(st))
        assert rc == ERR_ARG and not off and not ch and not soff and not sd and not st
    off, soff = u64p(), u64p()
    rc = L.awry_chain_batch(hostonly_index._h, qb.ctypes.data, qo.ctypes.data_as(u64p), 1, 12, 50, 100, 16, 100, 0, 1, C.byref(off), None, C.byref(soff), None, None)
    assert rc == ERR_ARG and not off and not soff


def test_cpp_mirror_method_compiles(tmp_path):
    src = tmp_path / "chains.cpp"
    src.write_text('#include <string>\n#include <vector>\n#include "awry.hpp"\n'
                   "uint64_t use(awry::FmIndex& ix) {\n"
                   '  std::vector<std::string> qs{"ACGTACGTACGT", "GATTACAGATTACA"};\n'
                   "  uint64_t s = 0;\n"
                   "  std::vector<uint8_t> status;\n"
                   "  awry::FmIndex::ChainParams p;\n"
                   "  p.lookback = 16;\n"
                   "  for (auto& per : ix.parallel_chains(qs, 12, 50, p, &status))\n"
                   "    for (const awry::FmIndex::Chain& c : per) {\n"
                   "      s += c.score + c.q_begin + c.q_end + c.t_begin + c.t_end;\n"
                   "      for (const awry_seed_t& m : c.seeds) s += m.q_begin + m.q_len + m.t_pos;\n"
                   "    }\n"
                   "  for (uint8_t st : status) s += st == AWRY_Q_SEED_CAP;\n"
                   "  static_assert(sizeof(awry_seed_t) == 16 && sizeof(awry_chain_t) == 32 && AWRY_CHAIN_MAX_SEEDS == 4096, \"layout\");\n"
                   "  return s + ix.parallel_chains(qs).size();\n}\n")
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"), str(src)])
