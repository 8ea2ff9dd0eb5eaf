"""Chain alignment without a GPU: the two forms of tests/chain_align_ref.py agree on random chains, the properties the header states
hold against an unbanded table, the CIGAR replays, the diagonal-first rule puts a deletion where the header says, the C ABI, ctypes,
the C++ mirror and the Rust sys crate agree, and the argument / no-replica errors come back as status codes."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from awry_amd import _lib
from awry_amd.fm_index import (ALN_BAD_CHAIN, ALN_DTYPE, ALN_OK, ALN_SKEW, BUILD_HOST, CHAIN_ALIGN_MAX_BAND, CHAIN_ALIGN_MAX_LEN, CHAIN_ALIGN_MAX_SKEW,
                               ERR_ARG, ERR_NO_DEVICE, AwryError, FmIndex, pack_queries)
from tests import chain_align_ref as ca
from tests import mismatch_ref as mr
from tests import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("awry_align_chains_batch", "awry_dev_align_chains", "awry_dev_align_chains_tally")
BANDS = (0, 1, 4, 8)


def sym(x):
    return [int(v) for v in mr.to_symbols(bytes(x), 0)]


@pytest.fixture(scope="module")
def text():
    t, st, _ = synth.make_text(3_000, 0, 5, 2, 0.04)  # two records (a join inside) and N runs
    assert len(st) == 2 and b"N" in bytes(t)
    return bytes(t), sym(t)[:-1], int(st[1])


def mutate(rng, s, rate):
    out = bytearray()
    for c in s:
        r = rng.random()
        if r < rate / 3:
            continue
        if r < 2 * rate / 3:
            out.append(int(synth.NT[rng.integers(0, 4)]))
            continue
        if r < rate:
            out += bytes([c, int(synth.NT[rng.integers(0, 4)])])
            continue
        out.append(c)
    return bytes(out) or b"A"


def random_case(rng, tb, n, join):
    """a read cut from the text (often near its ends, the join or an N run) with edits, and a member list along its diagonal:
    proper seeds, then members made to overlap, to be swallowed, to be unsorted or to reach out of range"""
    L0 = int(rng.choice([1, 2, 5, 17, 30, 48, 64])) + int(rng.integers(0, 8))
    where = rng.random()
    p = (0 if where < 0.1 else n - L0 if where < 0.2 else join - L0 // 2 if where < 0.3 else int(rng.integers(0, n - L0)))
    p = max(0, min(n - L0, p + int(rng.integers(-3, 4))))
    q = mutate(rng, tb[p:p + L0], float(rng.choice([0.0, 0.05, 0.15])))
    if rng.random() < 0.1:
        q = b"ACGTN"[int(rng.integers(0, 5)):][:1] * int(rng.integers(1, 6)) + q  # a read hanging over / an N against the text
    L = len(q)
    members, qb = [], int(rng.integers(0, max(1, L // 3 + 1)))
    while qb < L and len(members) < 6:
        ln = int(rng.integers(1, max(2, L // 3 + 1)))
        ln = min(ln, L - qb)
        tp = p + qb + int(rng.integers(-2, 3))
        members.append((qb, ln, tp))
        qb += ln + int(rng.integers(-3, 12))
        qb = max(qb, members[-1][0] + 1)
    kind = rng.random()
    if kind < 0.08 and len(members) > 1:
        members[0], members[1] = members[1], members[0]  # unsorted
    elif kind < 0.14:
        members.append((L - 1, 3, members[-1][2] + 40))  # past L
    elif kind < 0.2:
        members.append((L - 1, 1, n))  # past n
    elif kind < 0.24:
        members = []
    elif kind < 0.4 and members:
        a = members[int(rng.integers(0, len(members)))]
        members.append((a[0] + 1, max(1, a[1] // 2), a[2] + 1))  # swallowed by (or overlapping) the member it follows
        members.sort(key=lambda m: (m[0], m[2]))
    elif kind < 0.5 and members:
        members.append((members[-1][0] + 2, 2, members[-1][2] + int(rng.integers(15, 40))))  # a far member: a wide gap or a skew
    members = [(qb, ln, max(0, tp)) for qb, ln, tp in members]
    return q, members


@pytest.fixture(scope="module")
def random_cases(text):
    tb, ts, join = text
    rng = np.random.default_rng(2025)
    return [random_case(rng, tb, len(ts), join) + (BANDS[i % 4],) for i in range(2200)]


def test_the_two_forms_agree_on_2000_random_chains(text, random_cases):
    _, ts, _ = text
    assert len(random_cases) >= 2000
    seen = {ALN_OK: 0, ALN_SKEW: 0, ALN_BAD_CHAIN: 0}
    dropped = clipped = gaps = exts = wide = with_x = 0
    for q, members, W in random_cases:
        qs = sym(q)
        got = ca.align_chain(ts, qs, members, W)
        assert got == ca.align_chain(ts, qs, members, W, full=True), (q, members, W)
        st, tb, te, edits, runs, cells = got
        seen[st] += 1
        if st == ALN_OK:
            # replaying the CIGAR over q and T[t_begin .. t_end) reproduces both strings and the edit count
            assert ca.replay(qs, ts, tb, runs) == (len(qs), te, edits), (q, members, W)
            assert all(runs[k][1] != runs[k + 1][1] for k in range(len(runs) - 1)) and cells >= 0
            _, pcs = ca.pieces_of(members, len(qs), len(ts))
            dropped += len(pcs) < len(members)
            clipped += any(p not in members for p in pcs)
            gaps += len(pcs) > 1
            exts += pcs[0][0] > 0 or pcs[-1][0] + pcs[-1][1] < len(qs)
            wide += ca.widest_band(len(ts), len(qs), members, W) > 2 * W + 1
            with_x += any(c == "X" for _, c in runs)
            for (q0, l0, t0), (q1, _, t1) in zip(pcs, pcs[1:]):
                assert q0 + l0 <= q1 and t0 + l0 <= t1  # pieces overlap neither in the query nor in the text
        else:
            assert (edits, runs, cells) == (0, [], 0) and (st == ALN_SKEW or (tb, te) == (0, 0))
    assert seen[ALN_OK] > 1000 and seen[ALN_SKEW] > 30 and seen[ALN_BAD_CHAIN] > 200
    assert dropped > 50 and clipped > 50 and gaps > 500 and exts > 500 and wide > 200 and with_x > 200  # the cases do what they are for


def test_banded_costs_within_the_bounds_are_unbanded_optima(text):
    _, ts, _ = text
    rng = np.random.default_rng(7)
    tb = bytes(text[0])
    gap_exact = gap_over = ext_exact = ext_over = 0
    for it in range(600):
        W = BANDS[it % 4]
        a = int(rng.integers(0, 30))
        p = int(rng.integers(0, len(ts) - 80))
        x = sym(mutate(rng, tb[p:p + a], float(rng.choice([0.0, 0.1, 0.3]))) if a else b"")
        a = len(x)
        # a gap: any b with |b - a| <= MAX_SKEW
        b = max(0, a + int(rng.integers(-6, 7)))
        y = ts[p:p + b]
        v, _, _ = ca.segment(x, y, b, b - a, W, b)
        best = ca.unbanded(x, y, b)[a][b]
        assert v >= best
        if v <= abs(b - a) + 2 * W + 1:
            assert v == best
            gap_exact += 1
        else:
            gap_over += 1
        # an extension with avail >= a
        avail = a + 40
        J = min(a + W, avail)
        v, jstar, _ = ca.segment(x, ts[p:p + J], J, 0, W, None)
        row = ca.unbanded(x, ts[p:p + avail], avail)[a]
        assert v >= min(row)
        if v <= W:
            assert v == min(row) and jstar == row.index(v)
            ext_exact += 1
        else:
            ext_over += 1
    assert gap_exact > 300 and ext_exact > 100 and ext_over > 100


def plain(qb, tb, members, W):
    st, t_begin, t_end, edits, runs, _ = ca.align_chain(sym(tb), sym(qb), members, W)
    again = ca.align_chain(sym(tb), sym(qb), members, W, full=True)
    assert (st, t_begin, t_end, edits, runs) == again[:5]
    return st, t_begin, t_end, edits, ca.cigar_text(runs)


def test_a_deleted_unit_lands_where_the_diagonal_first_rule_puts_it():
    # a gap: the traceback from the gap's end takes the diagonal while it can, so the 'D's open the gap, right after the piece
    T, q = b"GGGGG" + b"AC" * 10 + b"TTTTT", b"AC" * 9
    assert plain(q, T, [(0, 4, 5), (14, 4, 21)], 4) == (ALN_OK, 5, 25, 2, "4=2D14=")
    # a left extension works on reversed strings: its traceback starts at the read's first letter and takes the diagonal while it
    # can, so the 'D's close the extension, right before the piece
    T, q = b"GTCAG" + b"AC" * 10 + b"TT", b"GTCAG" + b"AC" * 9
    assert plain(q, T, [(19, 4, 21)], 4) == (ALN_OK, 0, 25, 2, "19=2D4=")
    # without the anchoring flank the extension simply begins two letters later: no edit at all
    assert plain(b"AC" * 9, T, [(14, 4, 21)], 4) == (ALN_OK, 7, 25, 0, "18=")
    # the right extension mirrors the gap: '=' first from the end, the 'D's right after the piece
    T, q = b"TT" + b"AC" * 10 + b"GTCAG", b"AC" * 9 + b"GTCAG"
    assert plain(q, T, [(0, 4, 2)], 4) == (ALN_OK, 2, 27, 2, "4=2D19=")


def test_small_scripts_by_hand():
    T = b"ACGTACGTTTGACCA"
    assert plain(b"ACGTACGT", T, [(0, 8, 0)], 0) == (ALN_OK, 0, 8, 0, "8=")
    assert plain(b"ACGAACGT", T, [(0, 8, 0)], 4) == (ALN_OK, 0, 8, 1, "3=1X4=")  # a caller's seed that is no exact match
    assert plain(b"CGTACGTT", T, [(3, 2, 4)], 2) == (ALN_OK, 1, 9, 0, "8=")       # both extensions
    assert plain(b"GGACGT", T, [(2, 4, 0)], 1) == (ALN_OK, 0, 4, 2, "2I4=")        # hanging two letters over the start
    assert plain(b"ACCAGG", T, [(0, 4, 11)], 1) == (ALN_OK, 11, 15, 2, "4=2I")     # and over the end
    assert plain(b"ACGTACGT", T, [(0, 3, 0), (1, 3, 1), (5, 3, 5)], 1) == (ALN_OK, 0, 8, 0, "8=")  # a swallowed member, then a gap
    assert plain(b"ACGTACGT", T, [(0, 4, 0), (2, 6, 2)], 1) == (ALN_OK, 0, 8, 0, "8=")               # overlap in both: clipped
    assert plain(b"ACGT", T, [], 1)[0] == ALN_BAD_CHAIN and plain(b"ACGT", T, [(1, 2, 1), (0, 1, 0)], 1)[0] == ALN_BAD_CHAIN
    assert plain(b"ACGT", T, [(2, 3, 2)], 1)[0] == ALN_BAD_CHAIN and plain(b"ACGT", T, [(0, 4, 12)], 1)[0] == ALN_BAD_CHAIN
    q = b"A" * 17 + b"ACGT"
    assert plain(q, T, [(17, 4, 0)], 8)[:4] == (ALN_SKEW, 0, 4, 0) and plain(q[1:], T, [(16, 4, 0)], 8)[0] == ALN_OK  # 17 over the start; 16
    q = b"ACGT" + b"C" * 20 + b"CCA"
    assert plain(q, T, [(0, 4, 0), (24, 3, 7)], 8)[:4] == (ALN_SKEW, 0, 10, 0) and plain(q, T, [(0, 4, 0), (24, 3, 8)], 8)[0] == ALN_OK  # a gap of skew -17; -16
    assert plain(b"NACGT", b"NACGTNN", [(1, 4, 1)], 1) == (ALN_OK, 0, 5, 0, "5=")  # query N equals text N


def test_header_ctypes_cpp_mirror_and_rust_agree():
    L = _lib.load_library()
    for name in ENTRY_POINTS:
        assert name in _lib.header_symbols(), name
        assert getattr(L, name) is not None, name
    header = open(os.path.join(ROOT, "include", "awry_hip.h")).read()
    for word in ("AWRY_CHAIN_ALIGN_MAX_BAND = 8", "AWRY_CHAIN_ALIGN_MAX_SKEW = 16", "AWRY_CHAIN_ALIGN_MAX_LEN = 1024", "AWRY_ALN_OK = 0", "AWRY_ALN_SKEW = 1",
                 "AWRY_ALN_BAD_CHAIN = 2", "typedef struct { uint64_t t_begin, t_end; uint32_t edits, status; } awry_aln_t;"):
        assert word in header, word
    assert (CHAIN_ALIGN_MAX_BAND, CHAIN_ALIGN_MAX_SKEW, CHAIN_ALIGN_MAX_LEN) == (8, 16, 1024) == (ca.MAX_BAND, ca.MAX_SKEW, ca.MAX_LEN)
    assert (ALN_OK, ALN_SKEW, ALN_BAD_CHAIN) == (0, 1, 2) == (ca.ALN_OK, ca.ALN_SKEW, ca.ALN_BAD_CHAIN)
    assert C.sizeof(_lib.Aln) == 24 == ALN_DTYPE.itemsize == ca.ALN_NP.itemsize
    assert [(n, getattr(_lib.Aln, n).offset) for n, _ in _lib.Aln._fields_] == [(n, ALN_DTYPE.fields[n][1]) for n in ALN_DTYPE.names]
    src = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in ENTRY_POINTS:
        args = re.search(r"\b%s\s*\(([^)]*)\)" % name, src).group(1)
        assert len(args.split(",")) == len(getattr(L, name).argtypes), name
    rust = open(os.path.join(ROOT, "rust", "awry-hip-sys", "src", "lib.rs")).read()
    for word in ("pub struct awry_aln_t {\n    pub t_begin: u64,\n    pub t_end: u64,\n    pub edits: u32,\n    pub status: u32,\n}",
                 "pub fn awry_align_chains_batch(", "pub fn awry_dev_align_chains(", "pub fn awry_dev_align_chains_tally("):
        assert word in rust, word
    safe = open(os.path.join(ROOT, "rust", "awry", "src", "fm_index.rs")).read()
    assert "pub fn parallel_align_chains<'a>(" in safe and "sys::awry_align_chains_batch(" in safe


@pytest.fixture(scope="module")
def hostonly_index():
    t, st, hd = synth.make_text(2_000, 0, 61, 1, 0.0)
    return FmIndex.from_text(t, 0, 8, 0, st, hd, build_device=BUILD_HOST)  # no set_devices: no replica


def test_without_replicas_the_calls_return_no_device(hostonly_index):
    qb, qo = pack_queries([b"ACGTACGTACGT", b"GATTACA"])
    for call in (lambda: hostonly_index.parallel_align_chains_csr(qb, qo), lambda: hostonly_index.parallel_align_chains([b"ACGT"], min_len=1, max_hits=5),
                 lambda: hostonly_index.align_chains_string(b"ACGT"), lambda: hostonly_index.dev_align_chains(None, None, None, None, None, 0, 4, None, None),
                 lambda: hostonly_index.dev_align_chains_tally(None, None, None, None, None, 0, 4, None, None, None)):
        with pytest.raises(AwryError) as e:
            call()
        assert e.value.code == ERR_NO_DEVICE


def test_bad_parameters_are_argument_errors(hostonly_index):
    qb, qo = pack_queries([b"ACGTACGTACGT"])
    bad = [lambda: hostonly_index.parallel_align_chains_csr(qb, qo, band=9), lambda: hostonly_index.parallel_align_chains_csr(qb, qo, max_alignments=0),
           lambda: hostonly_index.parallel_align_chains_csr(qb, qo, min_len=0), lambda: hostonly_index.parallel_align_chains_csr(qb, qo, max_hits=0),
           lambda: hostonly_index.parallel_align_chains_csr(qb, qo, lookback=65), lambda: hostonly_index.parallel_align_chains_csr(qb, qo, max_seeds=0),
           lambda: hostonly_index.dev_align_chains(None, None, None, None, None, 0, 9, None, None),
           lambda: hostonly_index.dev_align_chains_tally(None, None, None, None, None, 0, 9, None, None, None)]
    for call in bad:
        with pytest.raises(AwryError) as e:
            call()
        assert e.value.code == ERR_ARG
    # the out-pointers of a failed call stay as they were; cigar_off_out without cigar_out is an argument error too
    L = _lib.load_library()
    u64p, u8p, u32p = C.POINTER(C.c_uint64), C.POINTER(C.c_uint8), C.POINTER(C.c_uint32)
    for tail in ((0, 4), (1, 9)):
        off, ch, al, coff, cg, st = u64p(), C.POINTER(_lib.Chain)(), C.POINTER(_lib.Aln)(), u64p(), u32p(), u8p()
        rc = L.awry_align_chains_batch(hostonly_index._h, qb.ctypes.data, qo.ctypes.data_as(u64p), 1, 12, 50, 100, 16, 100, 0, 1, *tail, C.byref(off),
                                       C.byref(ch), C.byref(al), C.byref(coff), C.byref(cg), C.byref(st))
        assert rc == ERR_ARG and not off and not ch and not al and not coff and not cg and not st
    off, coff = u64p(), u64p()
    rc = L.awry_align_chains_batch(hostonly_index._h, qb.ctypes.data, qo.ctypes.data_as(u64p), 1, 12, 50, 100, 16, 100, 0, 1, 1, 4, C.byref(off), None, None,
                                   C.byref(coff), None, None)
    assert rc == ERR_ARG and not off and not coff


def test_cpp_mirror_method_compiles(tmp_path):
    src = tmp_path / "align_chains.cpp"
    src.write_text('#include <string>\n#include <vector>\n#include "awry.hpp"\n'
                   "uint64_t use(awry::FmIndex& ix) {\n"
                   '  std::vector<std::string> qs{"ACGTACGTACGT", "GATTACAGATTACA"};\n'
                   "  uint64_t s = 0;\n"
                   "  std::vector<uint8_t> status;\n"
                   "  awry::FmIndex::ChainParams p;\n"
                   "  for (auto& per : ix.parallel_align_chains(qs, 12, 50, 3, 4, p, &status))\n"
                   "    for (const awry::FmIndex::ChainAlignment& a : per)\n"
                   "      s += a.chain.score + a.t_begin + a.t_end + a.edits + (a.status == AWRY_ALN_OK) + a.cigar.size() + a.cigar_string().size();\n"
                   "  static_assert(sizeof(awry_aln_t) == 24 && AWRY_CHAIN_ALIGN_MAX_BAND == 8 && AWRY_CHAIN_ALIGN_MAX_LEN == 1024, \"layout\");\n"
                   "  return s + ix.parallel_align_chains(qs).size();\n}\n")
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"), str(src)])
