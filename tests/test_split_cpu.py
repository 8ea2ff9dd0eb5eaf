"""Split reads without a GPU: the two forms of tests/split_ref.py agree on hand-made candidate lists and on 3 000 random reads whose
input meets stated conditions, properties 3 and 4 of the header hold there, every branch of the walk is built by hand, the C ABI,
ctypes, the C++ mirror and the Rust sys crate agree, and the argument / no-replica errors come back as status codes."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from awry_amd import _lib
from awry_amd.fm_index import (BUILD_HOST, ERR_ARG, ERR_NO_DEVICE, MAP_CLIP_DTYPE, MAP_SECONDARY, MAP_SPLIT_DTYPE, MAP_SUPPLEMENTARY, AwryError, FmIndex,
                               pack_queries, sa_tags)
from tests import clip_ref as cl
from tests import map_ref as mp
from tests import split_ref as sp
from tests import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("awry_map_split_batch", "awry_dev_map_select_split")
MAIN = (1, 4, 6, 5)
FRACTIONS = [(0, 1), (0, .6), (.6, 1), (0, .3), (.3, .6), (.55, 1), (.5, .5), (.6, .8), (.8, 1)]


def random_split_input(n, seed, n_text):
    """tests/test_clip_gpu.py's random_select_input (colliding spans, few distinct scores, a status mix) with a length per read and, for
    nine alignments in ten, clips that place the alignment on one of a few query intervals; the others keep their raw clips and saturate
    at small lengths.  -> (aln_off, alns, chains, chain_status, lengths)"""
    from tests.test_clip_gpu import random_select_input
    off, alns, chains, status = random_select_input(n, seed, n_text)
    rng = np.random.default_rng(seed + 1)
    lengths = rng.choice([0, 30, 41, 101, 150], size=n)
    tot = int(off[-1])
    query = np.repeat(np.arange(2 * n), np.diff(off).astype(np.int64))
    L = lengths[query >> 1]
    placed = rng.random(tot) < 0.9
    pick = rng.integers(0, len(FRACTIONS), size=tot)
    f = np.array(FRACTIONS)[pick]
    qb, qe = (f[:, 0] * L).astype(np.int64), (f[:, 1] * L).astype(np.int64)
    left = np.where(query % 2 == 0, qb, L - qe)
    right = np.where(query % 2 == 0, L - qe, qb)
    alns["clip_left"][:tot] = np.where(placed, left, alns["clip_left"][:tot])
    alns["clip_right"][:tot] = np.where(placed, right, alns["clip_right"][:tot])
    return off, alns, chains, status, lengths.astype(np.uint64)


@pytest.fixture(scope="module")
def random_reads():
    n, A = 3000, 8
    off, alns, chains, status, lengths = random_split_input(n, 7 * n + A, 40_000)
    cands = [sp.candidates_of(off, chains, alns, i, A) for i in range(n)]
    capped = [mp.Q_SEED_CAP in (int(status[2 * i]), int(status[2 * i + 1])) for i in range(n)]
    return n, cands, capped, [int(x) for x in lengths]


def test_the_random_input_exercises_every_branch(random_reads):
    n, cands, capped, lengths = random_reads
    got = [sp.walk(cands[i], capped[i], lengths[i], 4, 16, 50, MAIN, 0) for i in range(n)]
    seg = lambda recs: [r for r in recs if not r[7] & MAP_SECONDARY]
    two = sum(len(seg(r)) >= 2 for r, _ in got)
    three = sum(len(seg(r)) >= 3 for r, _ in got)
    four = sum(len(seg(r)) == 4 for r, _ in got)
    late_parent = sum(any(r[7] & MAP_SECONDARY and r[13] != 0 for r in recs) for recs, _ in got)
    mid_mapq = sum(any(0 < r[6] < 60 for r in seg(recs)) for recs, _ in got)
    empty = sum(s["empty"] > 0 for _, s in got)
    cap2 = sum(sp.walk(cands[i], capped[i], lengths[i], 2, 16, 50, MAIN, 0)[1]["capped"] > 0 for i in range(n))
    cap3 = sum(sp.walk(cands[i], capped[i], lengths[i], 3, 16, 50, MAIN, 0)[1]["capped"] > 0 for i in range(n))
    print("of %d reads: %d with >= 2 segments, %d with >= 3, %d with 4, %d with a secondary of a later segment, %d with a segment MAPQ in 1..59, "
          "%d drop an empty interval; %d drop a candidate at the cap at P = 2, %d at P = 3" % (n, two, three, four, late_parent, mid_mapq, empty, cap2, cap3))
    assert two >= 0.25 * n and three >= 0.04 * n and four >= 5 and late_parent >= 0.08 * n and mid_mapq >= 0.10 * n and empty >= 0.25 * n
    assert cap2 >= 0.02 * n and cap3 >= 5
    assert all(s["segments"] == len(seg(r)) and s["segments"] + s["secondaries"] == len(r) for r, s in got)  # R2 = 16 cuts nothing


@pytest.mark.parametrize("params", ((4, 16, 50, 0), (1, 0, 50, 0), (2, 1, 50, 30), (3, 2, 1, 0), (4, 16, 100, 31)))
def test_the_two_forms_agree_and_properties_3_and_4_hold_on_3000_random_reads(random_reads, params):
    n, cands, capped, lengths = random_reads
    P, R2, O, T = params
    for i in range(n):
        recs, stats = sp.walk(cands[i], capped[i], lengths[i], P, R2, O, MAIN, T)
        recs2, sets = sp.walk_matrix(cands[i], capped[i], lengths[i], P, R2, O, MAIN, T)
        assert recs == recs2, (i, params)
        segs = [r for r in recs if not r[7] & MAP_SECONDARY]
        assert len(segs) == stats["segments"] <= P and len(recs) == len(segs) + min(R2, stats["secondaries"])
        assert [r[13] for r in segs] == list(range(len(segs))) and [r[7] for r in segs] == ([0] + [MAP_SUPPLEMENTARY] * P)[:len(segs)]
        # (3) no two segments of a read overlap
        assert not any(sp.overlaps(a[11], a[12], b[11], b[12], O) for k, a in enumerate(segs) for b in segs[k + 1:]), (i, params)
        # (4) every secondary overlaps its parent, and no segment accepted before its parent
        for r in recs[len(segs):]:
            assert r[7] == MAP_SECONDARY and r[6] == 0 and r[14] == 0
            assert [x for x, g in enumerate(segs) if sp.overlaps(r[11], r[12], g[11], g[12], O)][0] == r[13], (i, params)
        assert all(min(s) == r[13] for s, r in zip(sets, recs[len(segs):]))
        assert all(r[12] > r[11] and r[8] >= T for r in recs)
        if P == 1 and recs:  # (5) the primary's MAPQ never falls below the clipped map level's
            clip, _ = cl.rank_candidates([c for c in cands[i] if sp.interval(c, lengths[i])[0] < sp.interval(c, lengths[i])[1]], capped[i], 1, MAIN, T)
            assert clip[0][:6] == recs[0][:6] and recs[0][6] >= clip[0][6], (i, params)


# ---- the branches of the walk, by hand --------------------------------------------------------------------------------------------------

def both(cands, capped, L, P, R2, O, wts=MAIN, T=0):
    recs, stats = sp.walk(cands, capped, L, P, R2, O, wts, T)
    assert recs == sp.walk_matrix(cands, capped, L, P, R2, O, wts, T)[0]
    return recs, stats


def brief(recs):
    """(t_begin, mapq, flags, q_begin, q_end, parent) per record"""
    return [(r[0], r[6], r[7], r[11], r[12], r[13]) for r in recs]


# (strand, j, edits, chain score, t_begin, t_end, score, clip_left, clip_right), L = 100
def test_an_exact_half_overlap_at_50_and_at_51_percent():
    a = (0, 0, 0, 60, 1000, 1060, 60, 0, 40)   # [0, 60)
    b = (0, 1, 2, 60, 5000, 5060, 50, 30, 10)  # [30, 90): 30 of 60 letters shared
    recs, _ = both([a, b], False, 100, 4, 16, 50)
    assert brief(recs) == [(1000, min(60, 10 * (60 - 50) // 5), 0, 0, 60, 0), (5000, 0, MAP_SECONDARY, 30, 90, 0)] and recs[0][6] == 20
    recs, _ = both([a, b], False, 100, 4, 16, 51)
    assert brief(recs) == [(1000, 60, 0, 0, 60, 0), (5000, 60, MAP_SUPPLEMENTARY, 30, 90, 1)]


def test_a_candidate_over_two_segments_belongs_to_the_first_accepted():
    g0 = (0, 0, 0, 50, 1000, 1050, 50, 50, 0)  # [50, 100), accepted first
    g1 = (0, 1, 0, 50, 5000, 5050, 45, 0, 50)  # [0, 50)
    c = (0, 2, 1, 50, 9000, 9065, 40, 10, 25)  # [10, 75): 25 letters of g0 (50 %), 40 of g1 (80 %)
    recs, stats = both([c, g1, g0], False, 100, 4, 16, 50)
    assert brief(recs) == [(1000, 20, 0, 50, 100, 0), (5000, 60, MAP_SUPPLEMENTARY, 0, 50, 1), (9000, 0, MAP_SECONDARY, 10, 75, 0)]
    assert stats == dict(empty=0, redundant=0, capped=0, segments=2, secondaries=1)
    recs, _ = both([c, g1, g0], False, 100, 4, 16, 51)  # no longer over g0: a secondary of g1, which gets the sub
    assert brief(recs) == [(1000, 60, 0, 50, 100, 0), (5000, 10, MAP_SUPPLEMENTARY, 0, 50, 1), (9000, 0, MAP_SECONDARY, 10, 75, 1)]
    recs, _ = both([c, g1, g0], False, 100, 4, 0, 51)  # only the report is cut: the sub stays
    assert brief(recs) == [(1000, 60, 0, 50, 100, 0), (5000, 10, MAP_SUPPLEMENTARY, 0, 50, 1)]


def test_the_segment_cap_drops_and_does_not_keep():
    a = (0, 0, 0, 60, 1000, 1060, 60, 0, 40)   # [0, 60)
    b = (0, 1, 0, 40, 5000, 5040, 40, 60, 0)   # [60, 100): a second segment, if there is room
    c = (0, 2, 3, 60, 5010, 5070, 30, 0, 40)   # [0, 60) again, at a place that intersects b's on the same strand
    recs, stats = both([a, b, c], False, 100, 2, 16, 50)
    assert brief(recs) == [(1000, 60, 0, 0, 60, 0), (5000, 60, MAP_SUPPLEMENTARY, 60, 100, 1)] and stats["redundant"] == 1 and stats["capped"] == 0
    recs, stats = both([a, b, c], False, 100, 1, 16, 50)  # b is dropped at the cap and is not kept: c is not redundant
    assert brief(recs) == [(1000, 10 * (60 - 30) // 5, 0, 0, 60, 0), (5010, 0, MAP_SECONDARY, 0, 60, 0)] and stats["capped"] == 1 and stats["redundant"] == 0


def test_an_empty_interval_and_saturated_clips():
    assert sp.interval((0, 0, 0, 0, 0, 0, 0, 60, 40), 100) == (60, 60) and sp.interval((0, 0, 0, 0, 0, 0, 0, 41, 30), 30) == (30, 30)
    assert sp.interval((0, 0, 0, 0, 0, 0, 0, 7, 41), 41) == (7, 7) and sp.interval((1, 0, 0, 0, 0, 0, 0, 7, 41), 41) == (41, 41)
    assert sp.interval((0, 0, 0, 0, 0, 0, 0, 0, 30), 0) == (0, 0) and sp.interval((0, 0, 0, 0, 0, 0, 0, 0, 0), 1 << 20) == (0, 0xFFFF)
    e = (0, 0, 0, 60, 1000, 1060, 99, 60, 40)   # explains no letter, the best score, on a's strand across a's span
    a = (0, 1, 0, 60, 1010, 1070, 60, 0, 40)
    recs, stats = both([e, a], False, 100, 4, 16, 50)
    assert brief(recs) == [(1010, 60, 0, 0, 60, 0)] and stats["empty"] == 1 and stats["redundant"] == 0  # no part in redundancy, no sub
    s = (0, 0, 0, 60, 1000, 1060, 99, 41, 30)   # clip_left + clip_right > L = 30: saturates to [30, 30)
    recs, stats = both([s, (0, 1, 0, 60, 1010, 1040, 30, 0, 0)], False, 30, 4, 16, 50)
    assert brief(recs) == [(1010, 60, 0, 0, 30, 0)] and stats["empty"] == 1


def test_text_redundancy_against_a_kept_secondary():
    a = (0, 0, 0, 100, 1000, 1100, 100, 0, 0)
    b = (0, 1, 2, 100, 5000, 5100, 90, 0, 0)   # a secondary of a
    c = (0, 2, 4, 100, 5050, 5150, 80, 0, 0)   # intersects b on strand 0: redundant
    recs, stats = both([a, b, c], False, 100, 4, 16, 50)
    assert brief(recs) == [(1000, 20, 0, 0, 100, 0), (5000, 0, MAP_SECONDARY, 0, 100, 0)] and stats["redundant"] == 1
    d = (1, 0, 4, 100, 5050, 5150, 80, 0, 0)   # the same span on the other strand
    assert [r[0] for r in both([a, b, d], False, 100, 4, 16, 50)[0]] == [1000, 5000, 5050]


def test_threshold_seed_cap_and_the_mirrored_interval_of_strand_1():
    a = (0, 0, 0, 100, 1000, 1100, 100, 0, 0)
    b = (0, 1, 2, 100, 5000, 5100, 90, 0, 0)
    assert brief(both([a, b], False, 100, 4, 16, 50, MAIN, 91)[0]) == [(1000, 60, 0, 0, 100, 0)]  # b is no candidate: no sub
    assert brief(both([a, b], False, 100, 4, 16, 50, MAIN, 101)[0]) == []
    assert [r[6] for r in both([a, b], True, 100, 4, 16, 50)[0]] == [0, 0]  # AWRY_Q_SEED_CAP
    assert [r[6] for r in both([a, b], False, 100, 4, 16, 50, (2, 3, 4, 0))[0]] == [20, 0] and [r[6] for r in both([a, b], False, 100, 4, 16, 50, (1, 0, 1, 0))[0]] == [60, 0]
    f = (0, 0, 0, 60, 1000, 1060, 60, 0, 40)   # strand 0: [0, 60)
    v = (1, 0, 0, 60, 5000, 5060, 59, 0, 40)   # strand 1, the same clips: [40, 100) of the read as given
    recs, _ = both([f, v], False, 100, 4, 16, 50)
    assert brief(recs) == [(1000, 60, 0, 0, 60, 0), (5000, 60, MAP_SUPPLEMENTARY, 40, 100, 1)] and recs[1][9:11] == (0, 40)  # the clips stay rc(read)'s
    v2 = (1, 0, 0, 60, 5000, 5060, 59, 40, 0)  # strand 1 with the clip on the left: [0, 60)
    assert brief(both([f, v2], False, 100, 4, 16, 50)[0]) == [(1000, 10 * (60 - 59) // 5, 0, 0, 60, 0), (5000, 0, MAP_SECONDARY, 0, 60, 0)]


def test_one_segment_is_the_clipped_map_level(random_reads):
    n, cands, capped, lengths = random_reads
    seen = 0
    for i in range(n):
        for R2 in (0, 2):
            recs, stats = sp.walk(cands[i], capped[i], lengths[i], 2, R2, 50, MAIN, 0)
            if stats["segments"] == 1 and stats["empty"] == 0:  # (2), where no candidate is dropped for an empty interval
                assert [r[:11] for r in recs] == cl.rank_candidates(cands[i], capped[i], 1 + R2, MAIN, 0)[0], i
                seen += 1
    assert seen > 200


def test_the_array_form_equals_the_list_form():
    alns = np.array([(1000, 1060, 0, 0, 60, 0, 41), (5000, 5041, 0, 0, 41, 60, 0), (7000, 7041, 1, 0, 36, 60, 0), (0, 0, 0, 2, 0, 0, 0), (9000, 9060, 0, 0, 60, 41, 0)],
                    cl.ALN_CLIP_NP)
    chains = np.zeros(5, [("score", "<u4")])
    chains["score"] = [60, 41, 41, 99, 60]
    off, rows, sel, st = sp.rank_alignments(np.array([0, 4, 5], np.uint64), chains, alns, [0, 0], [101], 1, 8, 4, 16, 50, MAIN, 0)
    assert list(off) == [0, 4] and sel == [0, 1, 4, 2] and list(st) == [0] and rows.dtype.itemsize == 48
    assert [tuple(int(v) for v in r) for r in rows] == [
        (1000, 1060, 0, 60, 0, 0, 0, 0, 60, 0, 41, 0, 60, 0, 0), (5000, 5041, 0, 41, 1, 0, 10, 16, 41, 60, 0, 60, 101, 1, 0),
        (9000, 9060, 0, 60, 0, 1, 0, 1, 60, 41, 0, 0, 60, 0, 0), (7000, 7041, 1, 41, 2, 0, 0, 1, 36, 60, 0, 60, 101, 1, 0)]
    assert sp.rank_alignments(np.array([0, 4, 5], np.uint64), chains, alns, [0, mp.Q_SEED_CAP], [101], 1, 1, 4, 16, 50, MAIN, 0)[1]["mapq"].tolist() == [0, 0]


def test_sa_tags_of_a_two_segment_read():
    recs = [(0, 499, 0, 60, 0, "60=41S", 0, 60, 0, 60, 0), (3, 99, 1, 10, 1, "39=1X1=60S", MAP_SUPPLEMENTARY, 36, 60, 101, 1),
            (2, 7, 0, 0, 2, "60S41=", MAP_SECONDARY, 31, 60, 101, 1)]
    assert sa_tags(recs, ["chr1", "chr2", "chr3", "chrX"]) == ["chrX,100,-,39=1X1=60S,10,1;", "chr1,500,+,60=41S,60,0;", None]
    assert sa_tags(recs[:1], ["chr1"]) == [""] and sa_tags([], []) == []
    three = recs[:2] + [(1, 0, 0, 60, 0, "90S11=", MAP_SUPPLEMENTARY, 11, 90, 101, 2)]
    assert sa_tags(three, ["a", "b", "c", "d"])[0] == "d,100,-,39=1X1=60S,10,1;b,1,+,90S11=,60,0;"


# ---- declarations ---------------------------------------------------------------------------------------------------------------------

def test_header_ctypes_cpp_mirror_and_rust_agree():
    L = _lib.load_library()
    for name in ENTRY_POINTS:
        assert name in _lib.header_symbols(), name
        assert getattr(L, name) is not None, name
    header = open(os.path.join(ROOT, "include", "awry_hip.h")).read()
    for word in ("AWRY_SPLIT_MAX_SEGMENTS = 4", "AWRY_MAP_SUPPLEMENTARY = 16", "uint16_t clip_left, clip_right; uint16_t q_begin, q_end, parent, reserved; } awry_map_split_t;",
                 "split reads: supplementary alignments by query overlap (no counterpart in the reference)", "100 ov >= O min(c.q_end - c.q_begin, g.q_end - g.q_begin)",
                 "q_end = max(q_begin, L - min(hi, L))", "No two segments of a read overlap", "that is intended"):
        assert word in header, word
    assert header.index("map read pairs, clipped: clipped pairing and rescue") < header.index("split reads: supplementary alignments by query overlap") < \
        header.index("releases an array one of the calls above")
    assert (sp.MAP_SUPPLEMENTARY, sp.MAX_SEGMENTS, MAP_SUPPLEMENTARY) == (16, 4, 16)
    assert C.sizeof(_lib.MapSplit) == 48 == MAP_SPLIT_DTYPE.itemsize == sp.MAP_SPLIT_NP.itemsize
    fields = [(n, getattr(_lib.MapSplit, n).offset) for n, _ in _lib.MapSplit._fields_]
    assert fields == [(n, MAP_SPLIT_DTYPE.fields[n][1]) for n in MAP_SPLIT_DTYPE.names] == [(n, sp.MAP_SPLIT_NP.fields[n][1]) for n in sp.MAP_SPLIT_NP.names]
    assert fields[:11] == [(n, MAP_CLIP_DTYPE.fields[n][1]) for n in MAP_CLIP_DTYPE.names] and fields[11:] == [("q_begin", 40), ("q_end", 42), ("parent", 44), ("reserved", 46)]
    src = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name, count in zip(ENTRY_POINTS, (27, 22)):
        args = re.search(r"\b%s\s*\(([^)]*)\)" % name, src).group(1)
        assert len(args.split(",")) == len(getattr(L, name).argtypes) == count, name
    rust = open(os.path.join(ROOT, "rust", "awry-hip-sys", "src", "lib.rs")).read()
    for word in ("pub struct awry_map_split_t {", "    pub clip_right: u16,\n    pub q_begin: u16,\n    pub q_end: u16,\n    pub parent: u16,\n    pub reserved: u16,\n}",
                 "pub const AWRY_MAP_SUPPLEMENTARY: u16 = 16;", "pub const AWRY_SPLIT_MAX_SEGMENTS: u32 = 4;") + tuple("pub fn %s(" % n for n in ENTRY_POINTS):
        assert word in rust, word
    assert "pub fn parallel_map_split" in open(os.path.join(ROOT, "rust", "awry", "src", "fm_index.rs")).read()
    for method in ("parallel_map_split_csr", "parallel_map_split", "map_split_string", "dev_map_select_split"):
        assert callable(getattr(FmIndex, method))


@pytest.fixture(scope="module")
def hostonly_index():
    t, st, hd = synth.make_text(2_000, 0, 61, 1, 0.0)
    return FmIndex.from_text(t, 0, 8, 0, st, hd, build_device=BUILD_HOST)  # no set_devices: no replica


def test_without_replicas_the_calls_return_no_device(hostonly_index):
    ix = hostonly_index
    qb, qo = pack_queries([b"ACGTACGTACGT", b"GATTACA"])
    for call in (lambda: ix.parallel_map_split_csr(qb, qo), lambda: ix.parallel_map_split([b"ACGT"], min_len=1), lambda: ix.map_split_string(b"ACGTACGT"),
                 lambda: ix.dev_map_select_split(None, None, None, None, None, 0, 4, 2, 1, 50, 1, 4, 0, None)):
        with pytest.raises(AwryError) as e:
            call()
        assert e.value.code == ERR_NO_DEVICE


def test_bad_parameters_are_argument_errors(hostonly_index):
    ix = hostonly_index
    qb, qo = pack_queries([b"ACGTACGTACGT"])
    for kw in (dict(max_segments=0), dict(max_segments=5), dict(chains_per_strand=2, max_secondary=5), dict(max_overlap=0), dict(max_overlap=101),
               dict(chains_per_strand=0), dict(chains_per_strand=9), dict(match=0), dict(match=17), dict(mismatch=65), dict(gap=65), dict(end_bonus=1025),
               dict(band=9), dict(min_len=0), dict(max_hits=0)):
        with pytest.raises(AwryError) as e:
            ix.parallel_map_split_csr(qb, qo, **kw)
        assert e.value.code == ERR_ARG, kw
    dev = lambda A=4, P=2, R2=1, O=50, a=1, b=4: ix.dev_map_select_split(None, None, None, None, None, 0, A, P, R2, O, a, b, 0, None)
    for kw in (dict(A=9), dict(A=0), dict(P=0), dict(P=5), dict(A=1, R2=3), dict(O=0), dict(O=101), dict(a=0), dict(a=17), dict(b=65)):
        with pytest.raises(AwryError) as e:
            dev(**kw)
        assert e.value.code == ERR_ARG, kw
    # the extreme values of every range are accepted: the call gets as far as the missing replica
    for kw in (dict(chains_per_strand=8, max_segments=4, max_secondary=16, max_overlap=100, match=16, mismatch=64, gap=64, end_bonus=1024, band=8),
               dict(chains_per_strand=1, max_segments=1, max_secondary=0, max_overlap=1, match=1, mismatch=0, gap=0, end_bonus=0, band=0)):
        with pytest.raises(AwryError) as e:
            ix.parallel_map_split_csr(qb, qo, min_aln_score=1 << 31, **kw)
        assert e.value.code == ERR_NO_DEVICE
    # the out-pointers of a failed call stay as they were
    L = _lib.load_library()
    u64p, u8p, u32p = C.POINTER(C.c_uint64), C.POINTER(C.c_uint8), C.POINTER(C.c_uint32)
    off, m, ps, coff, cg, st = u64p(), C.POINTER(_lib.MapSplit)(), C.POINTER(_lib.Pos)(), u64p(), u32p(), u8p()
    rc = L.awry_map_split_batch(ix._h, qb.ctypes.data, qo.ctypes.data_as(u64p), 1, 12, 50, 100, 16, 100, 10, 1, 4, 5, 0, 50, 4, 1, 4, 6, 5, 0, C.byref(off),
                                C.byref(m), C.byref(ps), C.byref(coff), C.byref(cg), C.byref(st))
    assert rc == ERR_ARG and not off and not m and not ps and not coff and not cg and not st


def test_cpp_mirror_methods_compile(tmp_path):
    src = tmp_path / "split.cpp"
    src.write_text('#include <string>\n#include <vector>\n#include "awry.hpp"\n'
                   "int64_t use(awry::FmIndex& ix) {\n"
                   '  std::vector<std::string> qs{"ACGTACGTACGT", "GATTACAGATTACA"};\n'
                   "  int64_t s = 0;\n"
                   "  std::vector<uint8_t> status;\n"
                   "  awry::FmIndex::ChainParams p;\n"
                   "  awry::FmIndex::ClipParams c;\n"
                   "  awry::FmIndex::SplitParams sp;\n"
                   "  sp.max_segments = 4;\n  sp.max_secondary = 2;\n  sp.max_overlap = 50;\n"
                   "  for (auto& per : ix.parallel_map_split(qs, 12, 50, 4, sp, 4, c, p, &status))\n"
                   "    for (const awry::FmIndex::SplitMapping& m : per)\n"
                   "      s += m.pos.seq_idx + m.map.t_end + m.map.score + m.map.mapq + m.map.q_begin + m.map.q_end + m.map.parent + m.cigar.size() +\n"
                   "           (m.supplementary() ? 1 : 0) + (m.secondary() ? 1 : 0);\n"
                   "  static_assert(sizeof(awry_map_split_t) == 48 && AWRY_MAP_SUPPLEMENTARY == 16 && AWRY_SPLIT_MAX_SEGMENTS == 4, \"layout\");\n"
                   '  return s + ix.map_split_string(qs[0]).size() + ix.map_split_string("ACGTACGT").size();\n}\n')
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"), str(src)])
