"""The clipped mode without a GPU: the two forms of tests/clip_ref.py agree on random chains, the five properties the header states
hold, the two sides of the end-bonus decision are built by hand, the pure ranking function and its MAPQ are checked on hand-made
candidate lists, the C ABI, ctypes, the C++ mirror and the Rust sys crate agree, and the argument / no-replica errors come back as
status codes."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from awry_amd import _lib
from awry_amd.fm_index import (ALN_CLIP_DTYPE, ALN_OK, BUILD_HOST, ERR_ARG, ERR_NO_DEVICE, MAP_CLIP_DTYPE, AwryError, FmIndex, cigar_string,
                               pack_queries)
from tests import chain_align_ref as ca
from tests import clip_ref as cl
from tests import map_ref as mp
from tests import synth
from tests.test_chain_align_cpu import random_case, sym

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("awry_align_chains_clip_batch", "awry_dev_align_chains_clip", "awry_dev_align_chains_clip_tally", "awry_map_clip_batch",
                "awry_dev_map_select_clip")
WEIGHTS = ((1, 4, 6), (2, 3, 4), (1, 1, 1), (1, 0, 1))  # (a, b, g); with the end bonuses below: (1,4,6,5), (2,3,4,0), (1,1,1,0), (1,0,1,0)
BONUS = (0, 5, 1024)
BANDS = (0, 1, 4, 8)


@pytest.fixture(scope="module")
def text():
    t, st, _ = synth.make_text(3_000, 0, 5, 3, 0.04)  # three records (two joins inside) and N runs
    assert len(st) == 3 and b"N" in bytes(t)
    return bytes(t), sym(t)[:-1], [int(v) for v in st]


def rec(starts, t):
    return max(k for k in range(len(starts)) if starts[k] <= t)


@pytest.fixture(scope="module")
def random_cases(text):
    tb, ts, st = text
    rng = np.random.default_rng(4242)
    out = []
    for i in range(2100):
        q, members = random_case(rng, tb, len(ts), st[1 + i % 2])
        if rng.random() < 0.4:  # a junk tail on either end, or on both: what the mode is for
            tail = lambda: bytes(int(synth.NT[rng.integers(0, 4)]) for _ in range(int(rng.choice([1, 3, 4, 5, 16, 30]))))
            side = rng.integers(0, 3)
            if side != 1:
                q = q + tail()
            if side != 0:
                head = tail()
                q, members = head + q, [(qb + len(head), ln, tp) for qb, ln, tp in members]
        w = WEIGHTS[(i // 4) % 4]
        E = (5, 0, 0, 0)[(i // 4) % 4] if i % 3 else BONUS[(i // 16) % 3]
        out.append((q, members, BANDS[i % 4], w + (E,)))
    return out


def test_the_two_forms_agree_on_2000_random_chains_and_properties_1_and_2_hold(text, random_cases):
    _, ts, st = text
    assert len(random_cases) >= 2000
    seen = {ca.ALN_OK: 0, ca.ALN_SKEW: 0, ca.ALN_BAD_CHAIN: 0}
    clipped = both = unclipped_ext = e2e_skew_ok = 0
    for q, members, W, wts in random_cases:
        qs = sym(q)
        got = cl.align_chain(ts, st, qs, members, W, wts)
        assert got == cl.align_chain(ts, st, qs, members, W, wts, full=True), (q, members, W, wts)
        status, tb, te, edits, runs, cells, score, c_l, c_r = got
        seen[status] += 1
        if status != ca.ALN_OK:
            assert (edits, runs, cells, score, c_l, c_r) == (0, [], 0, 0, 0, 0)
            continue
        # (1) replaying the CIGAR over q and T[t_begin .. t_end) reproduces both strings, edits, score and both clips
        consumed, t_end, r_edits, r_score, r_cl, r_cr = cl.replay(qs, ts, tb, runs, wts)
        assert (consumed, t_end, r_edits, r_score) == (len(qs), te, edits, score), (q, members, W, wts)
        assert r_cl + r_cr == c_l + c_r and ((r_cl, r_cr) == (c_l, c_r) or c_l + c_r == len(qs))
        assert all(c != "S" for _, c in runs[1:-1]) and sum(ln for ln, c in runs if c in "S=XI") == len(qs)
        assert all(runs[k][1] != runs[k + 1][1] or runs[k][1] == "S" for k in range(len(runs) - 1))
        assert score == wts[0] * sum(ln for ln, c in runs if c == "=") - wts[1] * sum(ln for ln, c in runs if c == "X") - \
            wts[2] * sum(ln for ln, c in runs if c in "ID")
        # (2) the aligned part lies in one record whenever the pieces do
        _, pcs = ca.pieces_of(members, len(qs), len(ts))
        if te > tb and rec(st, pcs[0][2]) == rec(st, max(pcs[0][2], pcs[-1][2] + pcs[-1][1] - 1)):
            assert rec(st, tb) == rec(st, te - 1) == rec(st, pcs[0][2]), (q, members, W, wts)
        clipped += c_l + c_r > 0
        both += c_l > 0 and c_r > 0
        unclipped_ext += c_l + c_r == 0 and (pcs[0][0] > 0 or pcs[-1][0] + pcs[-1][1] < len(qs))
        e2e_skew_ok += ca.align_chain(ts, qs, members, W)[0] == ca.ALN_SKEW
    assert seen[ca.ALN_OK] > 1000 and seen[ca.ALN_SKEW] > 10 and seen[ca.ALN_BAD_CHAIN] > 200
    assert clipped > 300 and both > 20 and unclipped_ext > 200 and e2e_skew_ok > 5  # the cases do what they are for


def test_properties_3_4_and_5_of_an_extension(text):
    _, ts, _ = text
    rng = np.random.default_rng(11)
    clipped = kept = 0
    for trial in range(1500):
        a_, b_, g_ = WEIGHTS[trial % 4]
        E, W = BONUS[(trial // 4) % 3], BANDS[(trial // 12) % 4]
        wts = (a_, b_, g_, E)
        a = int(rng.integers(1, 40))
        p = int(rng.integers(0, len(ts) - 60))
        good = int(rng.integers(0, a + 1))
        x = [s if s != 4 and k < good else int(rng.choice([1, 2, 3, 5])) for k, s in enumerate(ts[p:p + a])]
        avail = int(rng.choice([0, 1, a - W - 1, a, a + 20])) if rng.random() < 0.3 else a + 20
        J = min(a + W, max(0, avail))
        y = ts[p:p + J]
        ie, je, score, ops, (hstar, he) = cl.extension(x, y, J, W, wts)
        assert (ie, je, score, ops) == cl.extension(x, y, J, W, wts, full=True)[:4]
        assert hstar >= 0 and score == sum({"=": a_, "X": -b_, "I": -g_, "D": -g_}[c] for c in ops)
        # (5) clipped iff H* > H_e + E; the score is H* then and H_e otherwise, so it is at least H* - E >= -E, at least H_e, and at
        # least max(0, H_e) when E = 0 (an end-to-end extension that is kept may score below 0 by up to E: -8 at E = 1024 occurs here)
        assert (ie < a) == (he is None or hstar > he + E) and score == (hstar if ie < a else he)
        assert score >= hstar - E and (he is None or score >= he) and (E > 0 or score >= max(0, he if he is not None else 0))
        if ie < a:
            clipped += 1
            assert score == hstar
            if b_ >= 1 and g_ >= 1:  # (4) empty, or '=' at the outer end (the traceback's first operation)
                assert not ops or ops[0] == "=", (x, y, wts, ops)
        else:
            kept += 1
        # (3) an extension whose letters all match is never clipped
        if J >= a and all(cl.same(u, v) for u, v in zip(x, y)):
            assert ie == a and je == a and ops == ["="] * a
    assert clipped > 300 and kept > 300


def test_both_sides_of_the_end_bonus_decision(text):
    # ten matching letters, then one that differs, on the diagonal (W = 0): H* = 10 at (10, 10), H_e = 10 - 4 = 6 at (11, 11)
    T = sym(b"ACGTTGCAGTA" + b"CCCC")
    q = sym(b"ACGTTGCAGT" + b"C")
    for full in (False, True):
        ie, je, score, ops, (hstar, he) = cl.extension(q, T[:11], 11, 0, (1, 4, 6, 4), full)  # H_e + E = H*: not clipped
        assert (ie, je, score, hstar, he, "".join(ops)) == (11, 11, 6, 10, 6, "X" + "=" * 10)
        ie, je, score, ops, (hstar, he) = cl.extension(q, T[:11], 11, 0, (1, 4, 6, 3), full)  # H_e + E = H* - 1: clipped
        assert (ie, je, score, hstar, he, "".join(ops)) == (10, 10, 10, 10, 6, "=" * 10)
    # the same through a chain, as a right and as a left extension
    text_ = sym(b"GGGG" + b"ACGTTGCAGTA" + b"CCCC")
    read = sym(b"GGGG" + b"ACGTTGCAGT" + b"C")
    got = cl.align_chain(text_, [0], read, [(0, 4, 0)], 0, (1, 4, 6, 4))
    assert got[:5] == (ALN_OK, 0, 15, 1, [(14, "="), (1, "X")]) and got[6:] == (10, 0, 0)
    got = cl.align_chain(text_, [0], read, [(0, 4, 0)], 0, (1, 4, 6, 3))
    assert got[:5] == (ALN_OK, 0, 14, 0, [(14, "="), (1, "S")]) and got[6:] == (14, 0, 1)
    rtext, rread = text_[::-1], read[::-1]
    got = cl.align_chain(rtext, [0], rread, [(11, 4, 15)], 0, (1, 4, 6, 4))
    assert got[:5] == (ALN_OK, 4, 19, 1, [(1, "X"), (14, "=")]) and got[6:] == (10, 0, 0)
    got = cl.align_chain(rtext, [0], rread, [(11, 4, 15)], 0, (1, 4, 6, 3))
    assert got[:5] == (ALN_OK, 5, 19, 0, [(1, "S"), (14, "=")]) and got[6:] == (14, 1, 0)


def test_record_bounds_and_overhang_by_hand():
    # two records "ACGTACGTAC" and "GGTTGGTTGG" joined by N: a read over the join keeps to the record of its first piece
    T = sym(b"ACGTACGTAC" + b"N" + b"GGTTGGTTGG")
    st = [0, 11]
    q = sym(b"GTAC" + b"NGGTT")
    got = cl.align_chain(T, st, q, [(0, 4, 6)], 4, (1, 4, 6, 5))
    assert got[:5] == (ALN_OK, 6, 11, 0, [(5, "="), (4, "S")]) and got[6:] == (5, 0, 4)  # the join letter is the record's last
    assert ca.align_chain(T, q, [(0, 4, 6)], 4)[:4] == (ALN_OK, 6, 15, 0)  # end to end: into the next record
    got = cl.align_chain(T, st, sym(b"TTAC" + b"GGTT"), [(4, 4, 11)], 4, (1, 4, 6, 5))
    assert got[:5] == (ALN_OK, 11, 15, 0, [(4, "S"), (4, "=")]) and got[6:] == (4, 4, 0)  # avail = 0 on the left
    # a read hanging 20 letters over the text's end: AWRY_ALN_SKEW end to end, AWRY_ALN_OK and clipped here
    q = sym(b"GGTTGG" + b"ACGT" * 5)
    assert ca.align_chain(T, q, [(0, 4, 15)], 4)[0] == ca.ALN_SKEW
    got = cl.align_chain(T, st, q, [(0, 4, 15)], 4, (1, 4, 6, 5))
    assert got[:5] == (ALN_OK, 15, 21, 0, [(6, "="), (20, "S")]) and got[6:] == (6, 0, 20)
    assert cl.cigar_text(got[4]) == "6=20S" == cigar_string(cl.encode(got[4]))


def test_ranking_and_mapq_on_hand_made_candidates():
    W = (1, 4, 6, 5)
    # (strand, j, edits, chain score, t_begin, t_end, score, clip_left, clip_right)
    a = (0, 0, 2, 60, 1000, 1101, 91, 0, 0)
    b = (1, 0, 0, 50, 5000, 5070, 70, 0, 31)
    c = (0, 1, 1, 40, 1010, 1100, 85, 11, 0)  # intersects a on strand 0: redundant
    d = (1, 1, 0, 30, 1000, 1101, 91, 0, 0)   # a's span on the other strand, the same score, fewer edits: first
    recs, kept = cl.rank_candidates([a, b, c, d], False, 4, W, 0)
    assert kept == 3 and [r[:6] + r[8:] for r in recs] == [(1000, 1101, 0, 30, 1, 1, 91, 0, 0), (1000, 1101, 2, 60, 0, 0, 91, 0, 0),
                                                            (5000, 5070, 0, 50, 0, 1, 70, 0, 31)]
    assert [r[6] for r in recs] == [0, 0, 0] and [r[7] for r in recs] == [0, 1, 1]  # equal scores: MAPQ 0; secondaries flagged
    recs, kept = cl.rank_candidates([a, b], False, 1, W, 0)
    assert kept == 2 and len(recs) == 1 and recs[0][6] == min(60, 10 * (91 - 70) // 5) == 42
    assert cl.rank_candidates([a, b], True, 1, W, 0)[0][0][6] == 0  # the seed cap
    assert cl.rank_candidates([a], False, 2, W, 0)[0][0][6] == 60 and cl.rank_candidates([a, c], False, 2, W, 0)[1] == 1
    assert cl.rank_candidates([a, b], False, 2, W, 71)[0][0][6] == 60 and cl.rank_candidates([a, b], False, 2, W, 92) == ([], 0)  # the threshold
    assert cl.rank_candidates([a, b], False, 2, (2, 3, 4, 0), 0)[0][0][6] == 42 and cl.rank_candidates([a, b], False, 2, (1, 0, 1, 0), 0)[0][0][6] == 60
    e = (0, 2, 3, 10, 9000, 9100, 88, 0, 0)
    assert cl.rank_candidates([e, a], False, 2, (1, 1, 1, 0), 0)[0][0][6] == 10 * 3 // 2  # floor division
    # equal scores, no other difference but the edits, then the strand, then t_begin, then j
    f, g = (0, 0, 3, 10, 100, 200, 50, 0, 0), (0, 1, 2, 10, 300, 400, 50, 0, 0)
    assert [r[4] for r in cl.rank_candidates([f, g], False, 2, W, 0)[0]] == [1, 0]
    h = (0, 1, 3, 10, 50, 90, 50, 0, 0)
    assert [r[0] for r in cl.rank_candidates([f, h], False, 2, W, 0)[0]] == [50, 100]
    # the pure function over arrays equals the list form
    alns = np.array([(1000, 1101, 2, 0, 91, 0, 0), (1010, 1100, 1, 0, 85, 11, 0), (5000, 5070, 0, 0, 70, 0, 31), (1000, 1101, 0, 0, 91, 0, 0),
                     (0, 0, 0, 2, 0, 0, 0)], cl.ALN_CLIP_NP)
    chains = np.zeros(5, [("score", "<u4")])
    chains["score"] = [60, 40, 50, 30, 99]
    off, rows, sel, st = cl.rank_alignments(np.array([0, 2, 5], np.uint64), chains, alns, [0, 0], 1, 8, 4, W, 0)
    assert list(off) == [0, 3] and sel == [3, 0, 2] and list(st) == [0] and rows.dtype.itemsize == 40
    assert [tuple(int(v) for v in r) for r in rows] == [(1000, 1101, 0, 30, 1, 1, 0, 0, 91, 0, 0), (1000, 1101, 2, 60, 0, 0, 0, 1, 91, 0, 0),
                                                         (5000, 5070, 0, 50, 0, 1, 0, 1, 70, 0, 31)]
    assert cl.rank_alignments(np.array([0, 2, 5], np.uint64), chains, alns, [0, mp.Q_SEED_CAP], 1, 1, 4, W, 0)[1]["chain_index"].tolist() == [0, 0]


# ---- declarations ---------------------------------------------------------------------------------------------------------------------

def test_header_ctypes_cpp_mirror_and_rust_agree():
    L = _lib.load_library()
    for name in ENTRY_POINTS:
        assert name in _lib.header_symbols(), name
        assert getattr(L, name) is not None, name
    header = open(os.path.join(ROOT, "include", "awry_hip.h")).read()
    for word in ("AWRY_CLIP_MAX_MATCH = 16", "AWRY_CLIP_MAX_PENALTY = 64", "AWRY_CLIP_MAX_END_BONUS = 1024", "AWRY_CIGAR_SOFT_CLIP = 4",
                 "typedef struct { uint64_t t_begin, t_end; uint32_t edits, status; int32_t score; uint16_t clip_left, clip_right; } awry_aln_clip_t;",
                 "int32_t score; uint16_t clip_left, clip_right; } awry_map_clip_t;", "soft-clip read ends", "pairing clipped records is a later change",
                 "An extension whose letters all match is", "rec(t_begin) == rec(t_end - 1)"):
        assert word in header, word
    assert header.index("map reads on both strands") < header.index("soft-clip read ends: scored local extension") < header.index("map read pairs: insert-size pairing")
    assert (cl.MAX_MATCH, cl.MAX_PENALTY, cl.MAX_END_BONUS, cl.OP_CODE["S"]) == (16, 64, 1024, 4)
    assert C.sizeof(_lib.AlnClip) == 32 == ALN_CLIP_DTYPE.itemsize == cl.ALN_CLIP_NP.itemsize
    assert C.sizeof(_lib.MapClip) == 40 == MAP_CLIP_DTYPE.itemsize == cl.MAP_CLIP_NP.itemsize
    for ct, dt, ref in ((_lib.AlnClip, ALN_CLIP_DTYPE, cl.ALN_CLIP_NP), (_lib.MapClip, MAP_CLIP_DTYPE, cl.MAP_CLIP_NP)):
        assert [(n, getattr(ct, n).offset) for n, _ in ct._fields_] == [(n, dt.fields[n][1]) for n in dt.names] == [(n, ref.fields[n][1]) for n in ref.names]
    src = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in ENTRY_POINTS:
        args = re.search(r"\b%s\s*\(([^)]*)\)" % name, src).group(1)
        assert len(args.split(",")) == len(getattr(L, name).argtypes), name
    rust = open(os.path.join(ROOT, "rust", "awry-hip-sys", "src", "lib.rs")).read()
    for word in ("pub struct awry_aln_clip_t {\n    pub t_begin: u64,\n    pub t_end: u64,\n    pub edits: u32,\n    pub status: u32,\n    pub score: i32,\n"
                 "    pub clip_left: u16,\n    pub clip_right: u16,\n}", "pub struct awry_map_clip_t {", "pub const AWRY_CIGAR_SOFT_CLIP: u32 = 4;") + \
            tuple("pub fn %s(" % n for n in ENTRY_POINTS):
        assert word in rust, word
    for method in ("parallel_align_chains_clip_csr", "parallel_align_chains_clip", "parallel_map_clip_csr", "parallel_map_clip", "map_clip_string",
                   "dev_align_chains_clip", "dev_map_select_clip"):
        assert callable(getattr(FmIndex, method))
    assert cigar_string([3 << 4 | 4, 70 << 4 | 7, 1 << 4 | 8, 27 << 4 | 4]) == "3S70=1X27S"


@pytest.fixture(scope="module")
def hostonly_index():
    t, st, hd = synth.make_text(2_000, 0, 61, 1, 0.0)
    return FmIndex.from_text(t, 0, 8, 0, st, hd, build_device=BUILD_HOST)  # no set_devices: no replica


def test_without_replicas_the_calls_return_no_device(hostonly_index):
    ix = hostonly_index
    qb, qo = pack_queries([b"ACGTACGTACGT", b"GATTACA"])
    for call in (lambda: ix.parallel_align_chains_clip_csr(qb, qo), lambda: ix.parallel_align_chains_clip([b"ACGT"], min_len=1, max_hits=5),
                 lambda: ix.parallel_map_clip_csr(qb, qo), lambda: ix.parallel_map_clip([b"ACGT"], min_len=1), lambda: ix.map_clip_string(b"ACGTACGT"),
                 lambda: ix.dev_align_chains_clip(None, None, None, None, None, 0, 4, 1, 4, 6, 5, None, None),
                 lambda: ix.dev_map_select_clip(None, None, None, None, 0, 4, 1, 1, 4, 6, 5, 0, None)):
        with pytest.raises(AwryError) as e:
            call()
        assert e.value.code == ERR_NO_DEVICE


def test_bad_parameters_are_argument_errors(hostonly_index):
    ix = hostonly_index
    qb, qo = pack_queries([b"ACGTACGTACGT"])
    bad = [dict(match=0), dict(match=17), dict(mismatch=65), dict(gap=65), dict(end_bonus=1025), dict(band=9)]
    for kw in bad:
        for call in (lambda: ix.parallel_align_chains_clip_csr(qb, qo, **kw), lambda: ix.parallel_map_clip_csr(qb, qo, **kw)):
            with pytest.raises(AwryError) as e:
                call()
            assert e.value.code == ERR_ARG, kw
    for call in (lambda: ix.parallel_align_chains_clip_csr(qb, qo, max_alignments=0), lambda: ix.parallel_map_clip_csr(qb, qo, chains_per_strand=9),
                 lambda: ix.parallel_map_clip_csr(qb, qo, chains_per_strand=1, max_report=3), lambda: ix.parallel_map_clip_csr(qb, qo, min_len=0),
                 lambda: ix.dev_align_chains_clip(None, None, None, None, None, 0, 4, 0, 4, 6, 5, None, None),
                 lambda: ix.dev_align_chains_clip(None, None, None, None, None, 0, 9, 1, 4, 6, 5, None, None),
                 lambda: ix.dev_map_select_clip(None, None, None, None, 0, 4, 1, 1, 65, 6, 5, 0, None),
                 lambda: ix.dev_map_select_clip(None, None, None, None, 0, 4, 9, 1, 4, 6, 5, 0, None)):
        with pytest.raises(AwryError) as e:
            call()
        assert e.value.code == ERR_ARG
    # the extreme values of every range are accepted: the call gets as far as the missing replica
    for kw in (dict(match=16, mismatch=64, gap=64, end_bonus=1024), dict(match=1, mismatch=0, gap=0, end_bonus=0)):
        with pytest.raises(AwryError) as e:
            ix.parallel_map_clip_csr(qb, qo, min_aln_score=1 << 31, **kw)
        assert e.value.code == ERR_NO_DEVICE
    # the out-pointers of a failed call stay as they were
    L = _lib.load_library()
    u64p, u8p, u32p = C.POINTER(C.c_uint64), C.POINTER(C.c_uint8), C.POINTER(C.c_uint32)
    off, ch, al, coff, cg, st = u64p(), C.POINTER(_lib.Chain)(), C.POINTER(_lib.AlnClip)(), u64p(), u32p(), u8p()
    rc = L.awry_align_chains_clip_batch(ix._h, qb.ctypes.data, qo.ctypes.data_as(u64p), 1, 12, 50, 100, 16, 100, 0, 1, 1, 4, 0, 4, 6, 5, C.byref(off),
                                        C.byref(ch), C.byref(al), C.byref(coff), C.byref(cg), C.byref(st))
    assert rc == ERR_ARG and not off and not ch and not al and not coff and not cg and not st


def test_cpp_mirror_methods_compile(tmp_path):
    src = tmp_path / "clip.cpp"
    src.write_text('#include <string>\n#include <vector>\n#include "awry.hpp"\n'
                   "int64_t use(awry::FmIndex& ix) {\n"
                   '  std::vector<std::string> qs{"ACGTACGTACGT", "GATTACAGATTACA"};\n'
                   "  int64_t s = 0;\n"
                   "  std::vector<uint8_t> status;\n"
                   "  awry::FmIndex::ChainParams p;\n"
                   "  awry::FmIndex::ClipParams c;\n"
                   "  c.end_bonus = 0;\n"
                   "  for (auto& per : ix.parallel_align_chains_clip(qs, 12, 50, 3, 4, c, p, &status))\n"
                   "    for (const awry::FmIndex::ClippedChainAlignment& a : per)\n"
                   "      s += a.chain.score + a.aln.t_begin + a.aln.score + a.aln.clip_left + a.aln.clip_right + a.cigar_string().size();\n"
                   "  for (auto& per : ix.parallel_map_clip(qs, 12, 50, 4, 2, 4, c, p, &status))\n"
                   "    for (const awry::FmIndex::ClippedMapping& m : per)\n"
                   "      s += m.pos.seq_idx + m.map.t_end + m.map.score + m.map.mapq + m.map.clip_left + m.map.clip_right + m.cigar.size();\n"
                   "  static_assert(sizeof(awry_aln_clip_t) == 32 && sizeof(awry_map_clip_t) == 40 && AWRY_CIGAR_SOFT_CLIP == 4, \"layout\");\n"
                   '  return s + ix.map_clip_string(qs[0]).size() + ix.map_clip_string("ACGTACGT").size() + awry::FmIndex::cigar_text({3u << 4 | 4u}).size();\n}\n')
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"), str(src)])
