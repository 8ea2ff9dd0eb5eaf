"""Split reads on the GPU (kernels_split.hip.h) against tests/split_ref.py: the device primitive in both passes on random alignment
records that reach every branch of the walk -- every launch size, one and two blocks, two streams -- and awry_map_split_batch end to
end on reads of eight families over a text with planted two-copy repeats: against the reference, against the composition that needs
no reference, and against awry_map_clip_batch where the two must agree and where they must differ.  Everything must be equal: offsets,
records (every field), the selected alignments, positions, CIGAR runs, status."""
import ctypes as C
import os

import numpy as np
import pytest

from awry_amd.fm_index import (ALN_CLIP_DTYPE, CHAIN_DTYPE, ERR_ARG, ERR_INVALID_QUERY, MAP_CLIP_DTYPE, MAP_SECONDARY, MAP_SPLIT_DTYPE, MAP_SUPPLEMENTARY,
                               AwryError, FmIndex, cigar_string, pack_queries, sa_tags)
from tests import clip_ref as cl
from tests import map_ref as mp
from tests import mismatch_ref as mr
from tests import split_ref as sp
from tests import synth
from tests.test_chain_align_gpu import KEY, substitute
from tests.test_chain_gpu import E2E_PARAMS
from tests.test_clip_gpu import FAMILY, L_READ, families, rec_of
from tests.test_map_gpu import OracleWorld, positions_of
from tests.test_split_cpu import random_split_input

pytestmark = pytest.mark.gpu

MAIN = (1, 4, 6, 5)
P_MAIN = E2E_PARAMS[KEY]
PLANTS, PLANT_LEN, PLANT_SUBST = 12, 150, (40, 50, 60, 100)
# the places of the plants: a seed at which no read of tests/test_clip_gpu.py's families has a 41-letter half inside the letters 101 ..
# 149 of a plant, which both copies share (seed 12 puts one chimera there: two equal supplementaries, MAPQ 0)
PLANT_SEED = 15
O_MAIN = 50


def symbols(x):
    return [int(v) for v in mr.to_symbols(bytes(x), 0)]


# ---- the text: tests/test_clip_gpu.py's, with twelve two-copy repeats planted ---------------------------------------------------------

def planted_text():
    """-> (text, record starts, headers, [(source, copy)]): twelve clean 150-letter windows, each copied onto another clean window with
    the copy's letters at offsets 40, 50, 60 and 100 substituted"""
    text, st, hd = synth.make_text(40_000, 0, 21, 5, 0.03)
    text = np.array(text, copy=True)
    n = len(text) - 1
    ends = [int(v) for v in st] + [n]
    rng = np.random.default_rng(PLANT_SEED)
    taken, plants = [], []

    def window():
        while True:
            p = int(rng.integers(0, n - PLANT_LEN))
            r = rec_of(ends[:-1], p)
            clean = all(c in b"ACGT" for c in bytes(text[p:p + PLANT_LEN]))
            if clean and p + PLANT_LEN < ends[r + 1] - 1 and all(p + PLANT_LEN + 20 <= a or a + PLANT_LEN + 20 <= p for a in taken):
                taken.append(p)
                return p

    for _ in range(PLANTS):
        src, dst = window(), window()
        text[dst:dst + PLANT_LEN] = np.frombuffer(substitute(bytes(text[src:src + PLANT_LEN]), PLANT_SUBST), np.uint8)
        plants.append((src, dst))
    return text, st, hd, plants


class SplitWorld(OracleWorld):
    """OracleWorld over the planted text; device=False builds no GPU index (the reference-only conditions need none)"""

    def __init__(self, oracle, device=True):
        text, st, hd, self.plants = planted_text()
        self.text, self.st, self.hd, self.alphabet = text, st, hd, 0
        self.ix = FmIndex.from_text(text, 0, 8, 0, st, hd).set_devices([0]) if device else None
        self.oi = oracle.OracleIndex.from_text(text, 0, 8, 0, st, hd)
        self._ref, self._chains = {}, {}
        self.tsym = symbols(text)[:-1]
        self.starts = [int(v) for v in st]


def all_families(w):
    """tests/test_clip_gpu.py's six families on this text, and two per planted repeat; every second read reverse-complemented"""
    fam = families(w)
    tb = bytes(w.text[:-1])
    rng = np.random.default_rng(4)
    inside = lambda p, L: any(a < p + L and p < a + PLANT_LEN for pair in w.plants for a in pair)
    rep, chim = [], []
    for src, dst in w.plants:
        q = bytearray(tb[src + 25:src + 126])
        q[75] = tb[dst + 100]  # one letter of the copy: both copies are seeded
        rep.append((bytes(q), src + 25, dst + 25))
        while True:
            p = int(rng.integers(0, len(tb) - 60))
            if all(c in b"ACGT" for c in tb[p:p + 60]) and not inside(p, 60) and rec_of(w.starts, p) == rec_of(w.starts, p + 59):
                break
        part = bytearray(tb[src + 30:src + 71])
        part[10] = tb[dst + 40]
        chim.append((tb[p:p + 60] + bytes(part), p, (src + 30, dst + 30)))
    for name, rows in (("repeat", rep), ("chimera-repeat", chim)):
        fam[name] = [(mp.rc(q) if i % 2 else q, i % 2, origin, extra) for i, (q, origin, extra) in enumerate(rows)]
        assert all(len(r[0]) == L_READ for r in fam[name])
    return fam


def reference_conditions(w, fam, memo):
    """what the families are for, from the reference alone, at A = 3 and A = 8"""
    seg = lambda recs: [r for r in recs if not r[7] & MAP_SECONDARY]
    for A in (3, 8):
        per = {name: sp.map_reads(w.tsym, w.starts, [r[0] for r in rows], w.chains_of(P_MAIN), A, 4, 2 * A, O_MAIN, 4, MAIN, 0, memo) for name, rows in fam.items()}
        for (q, strand, o_src, o_dst), (_, recs, _) in zip(fam["repeat"], per["repeat"]):
            assert [(r[0], r[8], r[6], r[7], r[13]) for r in recs] == [(o_src, 96, 20, 0, 0), (o_dst, 86, 0, MAP_SECONDARY, 0)], (A, recs)
        for (q, strand, p, (o_src, o_dst)), (_, recs, _) in zip(fam["chimera-repeat"], per["chimera-repeat"]):
            assert len(recs) == 3 and [r[7] for r in recs] == [0, MAP_SUPPLEMENTARY, MAP_SECONDARY] and [r[13] for r in recs] == [0, 1, 1], (A, recs)
            assert recs[0][0] == p and recs[0][6] == 60 and recs[0][8] >= 60
            assert recs[1][8] in (36, 37) and recs[1][6] == 10 and recs[2][8] == recs[1][8] - 5 and (recs[1][1], recs[2][1]) == (o_src + 41, o_dst + 41)
        for name in ("chimera", "join"):
            for row, (_, recs, _) in zip(fam[name], per[name]):
                s = seg(recs)
                assert len(s) == 2 and rec_of(w.starts, s[0][0]) != rec_of(w.starts, s[1][0]), (A, name, recs)
                if name == "chimera":
                    assert [r[6] for r in s] == [60, 60] and s[1][7] == MAP_SUPPLEMENTARY
                    first, second = sorted(s, key=lambda r: r[11])
                    cut = 60 if row[1] == 0 else L_READ - 60  # (a reversed read is rc(60 + 41): the 41 letters come first)
                    assert first[11] == 0 and second[12] == L_READ and abs(first[12] - cut) <= 4 and abs(second[11] - cut) <= 4, (A, recs)
        for name in ("exact", "subst", "tail", "end"):
            assert all(len(seg(recs)) == 1 for _, recs, _ in per[name]), (A, name)


# ---- the device primitive -------------------------------------------------------------------------------------------------------------------

PRIMITIVE_PARAMS = lambda A: ((1, 0, 50, 0, MAIN), (2, 1, 50, 30, MAIN), (3, 2, 50, 0, MAIN), (4, 2 * A, 1, 0, (2, 3, 4, 0)), (4, 2 * A, 100, 0, MAIN),
                              (4, 2 * A, 50, 31, (1, 0, 1, 0)))


def offsets_of(lengths):
    qoff = np.zeros(len(lengths) + 1, np.uint64)
    qoff[1:] = np.cumsum(lengths, dtype=np.uint64)
    return qoff


def split_job(ix, inp, A, params, tot, stream=None):
    """upload, and 0xEE behind every output array; the record arrays hold the most a read can get, n (P + R2) records, so that a wrong
    count pass shows as a difference and not as a write past the end"""
    off, alns, chains, status, lengths = inp
    n = len(lengths)
    want_tot, tot = tot, n * (params[0] + params[1])
    assert want_tot <= tot
    d = dict(n=n, A=A, params=params, tot=tot, s=stream, off=ix.dev_upload(off), al=ix.dev_upload(alns.view(np.uint8)), ch=ix.dev_upload(chains.view(np.uint8)),
             st=ix.dev_upload(status), qo=ix.dev_upload(offsets_of(lengths)), nm=ix.dev_malloc(8 * (n + 2)), rs=ix.dev_malloc(n + 8), mo=ix.dev_malloc(8 * (n + 1)),
             scr=ix.dev_malloc(ix.dev_scan_scratch_bytes(n)), mp=ix.dev_malloc(48 * (tot + 2)), sel=ix.dev_malloc(4 * (tot + 2)), pos=ix.dev_malloc(16 * (tot + 2)))
    for key, size in (("nm", 8 * (n + 2)), ("rs", n + 8), ("mp", 48 * (tot + 2)), ("sel", 4 * (tot + 2)), ("pos", 16 * (tot + 2))):
        ix.dev_memset(d[key], 0xEE, size)
    return d


def run_split_job(ix, d):
    """count pass, scan, fill pass, all queued on the job's stream (the fill pass writes within the reference's offsets: tot is theirs)"""
    P, R2, O, T, wts = d["params"]
    args = (d["off"], d["al"], d["ch"], d["st"], d["qo"], d["n"], d["A"], P, R2, O, wts[0], wts[1], T)
    ix.dev_map_select_split(*args, d["nm"], d["rs"], stream=d["s"])
    ix.dev_scan_counts(d["nm"], d["n"], d["mo"], d["scr"], d["s"])
    ix.dev_map_select_split(*args, None, None, d["mo"], d["mp"], d["sel"], d["pos"], stream=d["s"])


def split_result(ix, d):
    n, tot = d["n"], d["tot"]
    out = dict(mo=ix.dev_download(d["mo"], (n + 1,), np.uint64), nm=ix.dev_download(d["nm"], (n + 2,), np.uint64), rs=ix.dev_download(d["rs"], (n + 8,), np.uint8),
               mp=ix.dev_download(d["mp"], (48 * (tot + 2),), np.uint8), sel=ix.dev_download(d["sel"], (tot + 2,), np.uint32),
               pos=ix.dev_download(d["pos"], (tot + 2, 2), np.uint64))
    for key in ("off", "al", "ch", "st", "qo", "nm", "rs", "mo", "scr", "mp", "sel", "pos"):
        ix.dev_free(d[key])
    return out


def assert_split_select(got, want, st, what):
    woff, wrec, wsel, wst = want
    n, tot = len(wst), int(woff[-1])
    assert np.array_equal(got["mo"], woff), what
    assert np.array_equal(got["nm"][:n], np.diff(woff)) and np.all(got["nm"][n:] == 0xEEEEEEEEEEEEEEEE), what
    assert np.array_equal(got["rs"][:n], wst) and np.all(got["rs"][n:] == 0xEE), what
    g = got["mp"][:48 * tot].view(MAP_SPLIT_DTYPE)
    for f in MAP_SPLIT_DTYPE.names:
        bad = np.nonzero(g[f] != wrec[f])[0]
        assert not len(bad), (what, f, int(bad[0]), g[bad[0]], wrec[bad[0]])
    assert np.array_equal(got["sel"][:tot], np.array(wsel, np.uint32)) and np.array_equal(got["pos"][:tot], positions_of(st, wrec["t_begin"])), what
    assert np.all(got["mp"][48 * tot:] == 0xEE) and np.all(got["sel"][tot:] == 0xEEEEEEEE) and np.all(got["pos"][tot:] == 0xEEEEEEEEEEEEEEEE), what


@pytest.fixture(scope="module")
def nt(oracle):
    return SplitWorld(oracle)


@pytest.fixture(scope="module")
def select_cases(nt):
    """per (n, A): the random input and, per parameter set, the reference's answer; computed once"""
    memo = {}

    def get(n, A):
        if (n, A) not in memo:
            inp = random_split_input(n, 7 * n + A, len(nt.text) - 1)
            memo[(n, A)] = (inp, {p: sp.rank_alignments(inp[0], inp[2], inp[1], inp[3], inp[4], n, A, p[0], p[1], p[2], p[4], p[3]) for p in PRIMITIVE_PARAMS(A)})
        return memo[(n, A)]
    return get


@pytest.mark.parametrize("A", (1, 3, 8))
def test_split_select_equals_the_reference_in_both_passes(nt, select_cases, A):
    ix = nt.ix
    for n in (1, 257, 3000):
        inp, wants = select_cases(n, A)
        for params, want in wants.items():
            d = split_job(ix, inp, A, params, int(want[0][-1]))
            run_split_job(ix, d)
            ix.dev_synchronize()
            assert_split_select(split_result(ix, d), want, nt.st, (A, n, params))
        assert n == 1 or sum(int(w[0][-1]) for w in wants.values()) > n
    ix.dev_map_select_split(None, None, None, None, None, 0, A, 1, 0, 50, 1, 4, 0, None)  # no read: null pointers are fine


@pytest.mark.parametrize("blocks", (1, 2))
def test_split_select_past_one_grid_trip(nt, select_cases, blocks):
    import awry_amd
    L_ = awry_amd.load_library()
    inp, wants = select_cases(3000, 8)
    before = L_.awry_debug_max_blocks()
    L_.awry_debug_set_max_blocks(blocks)
    try:
        for params in PRIMITIVE_PARAMS(8)[2:5]:
            d = split_job(nt.ix, inp, 8, params, int(wants[params][0][-1]))
            run_split_job(nt.ix, d)
            nt.ix.dev_synchronize()
            assert_split_select(split_result(nt.ix, d), wants[params], nt.st, (blocks, params))
    finally:
        L_.awry_debug_set_max_blocks(before)


def test_two_streams_with_all_launches_queued_before_any_wait(nt, select_cases):
    import torch
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    plan = [(3000, 8, PRIMITIVE_PARAMS(8)[4]), (3000, 3, PRIMITIVE_PARAMS(3)[2])]
    jobs = []
    for (n, A, params), s in zip(plan, streams):
        inp, wants = select_cases(n, A)
        jobs.append((split_job(nt.ix, inp, A, params, int(wants[params][0][-1]), stream=s.cuda_stream), wants[params]))
    nt.ix.dev_synchronize()
    for d, _ in jobs:
        run_split_job(nt.ix, d)
    nt.ix.dev_synchronize()
    for d, want in jobs:
        assert_split_select(split_result(nt.ix, d), want, nt.st, d["params"])


# ---- the batch entry point ------------------------------------------------------------------------------------------------------------------

def want_split(w, reads, A, P, R2, W, wts, T, memo, O=O_MAIN):
    return sp.as_csr(sp.map_reads(w.tsym, w.starts, reads, w.chains_of(P_MAIN), A, P, R2, O, W, wts, T, memo))


def got_split(ix, reads, A, P, R2, W, wts, T, O=O_MAIN, **kw):
    return ix.parallel_map_split_csr(*pack_queries(reads), *KEY, A, P, R2, O, W, *wts, T, *P_MAIN, **kw)


def assert_split_equal(got, want, st, what=None):
    off, maps, pos, coff, cg, status = got
    woff, wrec, wcoff, wcg, wst = want
    assert maps.dtype == MAP_SPLIT_DTYPE
    assert np.array_equal(off, woff) and np.array_equal(status, wst), what
    for f in MAP_SPLIT_DTYPE.names:
        bad = np.nonzero(maps[f] != wrec[f])[0]
        assert not len(bad), (what, f, int(bad[0]), maps[bad[0]], wrec[bad[0]])
    assert np.array_equal(pos, positions_of(st, wrec["t_begin"])), what
    assert np.array_equal(coff, wcoff) and np.array_equal(cg, wcg), what


def composition(ix, reads, A, P, R2, W, wts, T, O=O_MAIN):
    """what needs no reference: awry_align_chains_clip_batch on the doubled batch built on the host, walked by the pure function"""
    off, ch, al, coff, cg, st = ix.parallel_align_chains_clip_csr(*pack_queries(mp.doubled(reads)), *KEY, A, W, *wts, *P_MAIN)
    assert ch.dtype == CHAIN_DTYPE and al.dtype == ALN_CLIP_DTYPE
    moff, rec, sel, rst = sp.rank_alignments(off, ch, al, st, [len(q) for q in reads], len(reads), A, P, R2, O, wts, T)
    runs = [cg[int(coff[c]):int(coff[c + 1])] for c in sel]
    wcoff = np.zeros(len(sel) + 1, np.uint64)
    wcoff[1:] = np.cumsum([len(r) for r in runs], dtype=np.uint64)
    return moff, rec, wcoff, np.concatenate(runs + [np.zeros(0, np.uint32)]).astype(np.uint32), rst


@pytest.fixture(scope="module")
def main(nt):
    fam = all_families(nt)
    reads = [r[0] for rows in fam.values() for r in rows]
    return fam, reads, {}


def test_the_reference_meets_the_conditions_the_families_are_for(nt, main):
    fam, _, memo = main
    assert len(fam) == 8 and len(fam["repeat"]) == len(fam["chimera-repeat"]) == PLANTS and len(fam["chimera"]) == FAMILY
    reference_conditions(nt, fam, memo)


@pytest.mark.parametrize("band", (0, 4, 8))
def test_batch_equals_the_reference_and_the_composition(nt, main, band):
    _, reads, memo = main
    for A, P, R2 in ((1, 1, 0), (3, 2, 2), (8, 4, 16)):
        for T in (0, 30):
            want = want_split(nt, reads, A, P, R2, band, MAIN, T, memo)
            got = got_split(nt.ix, reads, A, P, R2, band, MAIN, T)
            assert_split_equal(got, want, nt.st, (A, P, R2, band, T))
            assert_split_equal(got, composition(nt.ix, reads, A, P, R2, band, MAIN, T), nt.st, ("composition", A, P, R2, band, T))
            assert int(got[0][-1]) > len(reads) // 2


def query_letters(runs):
    return sum(int(v) >> 4 for v in runs if int(v) & 15 in (7, 8, 1))  # '=', 'X', 'I'


def test_properties_1_and_2_and_the_contrast_with_the_clipped_map_level(nt, main):
    fam, reads, _ = main
    A, P, R2 = 8, 4, 2
    off, maps, pos, coff, cg, status = got_split(nt.ix, reads, A, P, R2, 4, MAIN, 0)
    coff2, maps2, _, ccoff2, cg2, status2 = nt.ix.parallel_map_clip_csr(*pack_queries(reads), *KEY, A, 1 + R2, 4, *MAIN, 0, *P_MAIN)
    assert np.array_equal(status, status2)
    one_segment = 0
    for i, q in enumerate(reads):
        recs = range(int(off[i]), int(off[i + 1]))
        for c in recs:  # (1) the interval is the CIGAR's query letters, and follows from strand, clips and L
            m = maps[c]
            lo, hi = (int(m["clip_left"]), int(m["clip_right"])) if m["strand"] == 0 else (int(m["clip_right"]), int(m["clip_left"]))
            assert (int(m["q_begin"]), int(m["q_end"])) == (lo, len(q) - hi) and int(m["reserved"]) == 0
            assert int(m["q_end"]) - int(m["q_begin"]) == query_letters(cg[int(coff[c]):int(coff[c + 1])])
        segs = [c for c in recs if not maps[c]["flags"] & MAP_SECONDARY]
        if len(segs) == 1:  # (2) exactly what awry_map_clip_batch reports at max_report = 1 + R2
            one_segment += 1
            theirs = range(int(coff2[i]), int(coff2[i + 1]))
            assert len(theirs) == len(recs), i
            for c, c2 in zip(recs, theirs):
                assert all(maps[c][f] == maps2[c2][f] for f in MAP_CLIP_DTYPE.names), (i, maps[c], maps2[c2])
                assert np.array_equal(cg[int(coff[c]):int(coff[c + 1])], cg2[int(ccoff2[c2]):int(ccoff2[c2 + 1])])
    assert one_segment >= 4 * FAMILY
    # the contrast: the chimeras at the clipped map level (R = 2) and here
    lo = list(fam).index("chimera") * FAMILY
    m_off, m_maps = nt.ix.parallel_map_clip_csr(*pack_queries(reads[lo:lo + FAMILY]), *KEY, A, 2, 4, *MAIN, 0, *P_MAIN)[:2]
    for k in range(FAMILY):
        theirs = m_maps[int(m_off[k]):int(m_off[k + 1])]
        assert len(theirs) == 2 and theirs[0]["mapq"] < 60 and theirs[1]["flags"] == MAP_SECONDARY and theirs[1]["mapq"] == 0
        mine = maps[int(off[lo + k]):int(off[lo + k + 1])]
        assert [int(x) for x in mine["mapq"][:2]] == [60, 60] and [int(x) for x in mine["flags"][:2]] == [0, MAP_SUPPLEMENTARY]


def test_the_list_api_and_the_call_without_the_optional_arrays(nt, main):
    fam, reads, memo = main
    lo = list(fam).index("chimera") * FAMILY
    sub = reads[lo:lo + 3] + [fam["chimera-repeat"][0][0]]
    woff, wrec, wcoff, wcg, _ = want_split(nt, sub, 3, 2, 2, 4, MAIN, 0, memo)
    pos = positions_of(nt.st, wrec["t_begin"])
    want = [[(int(pos[c][0]), int(pos[c][1]), int(wrec[c]["strand"]), int(wrec[c]["mapq"]), int(wrec[c]["edits"]),
              cigar_string(wcg[int(wcoff[c]):int(wcoff[c + 1])]), int(wrec[c]["flags"]), int(wrec[c]["score"]), int(wrec[c]["q_begin"]), int(wrec[c]["q_end"]),
              int(wrec[c]["parent"])) for c in range(int(woff[i]), int(woff[i + 1]))] for i in range(4)]
    assert nt.ix.parallel_map_split(sub, *KEY, 3, 2, 2, O_MAIN, 4, *MAIN, 0, **P_MAIN._asdict()) == want and [len(x) for x in want] == [2, 2, 2, 3]
    assert nt.ix.map_split_string(sub[3], *KEY, 3, 2, 2, O_MAIN, 4, *MAIN, 0, **P_MAIN._asdict()) == want[3]
    tags = sa_tags(want[3], nt.hd)
    assert tags[2] is None and tags[0].count(";") == 1 and tags[0].split(",")[3] == want[3][1][5] and tags[1].split(",")[4] == "60"
    full = got_split(nt.ix, reads, 3, 2, 2, 4, MAIN, 0)
    bare = got_split(nt.ix, reads, 3, 2, 2, 4, MAIN, 0, want_pos=False, want_cigar=False)
    assert np.array_equal(bare[0], full[0]) and np.array_equal(bare[1], full[1]) and np.array_equal(bare[5], full[5])
    assert len(bare[2]) == 0 and len(bare[3]) == 0 and len(bare[4]) == 0


def test_results_do_not_depend_on_capacity_sub_batch_replicas_table_or_grid(nt, main):
    import awry_amd
    import torch
    _, reads, memo = main
    want = want_split(nt, reads, 8, 4, 16, 4, MAIN, 0, memo)
    L_ = awry_amd.load_library()

    def check(ix, name):
        assert_split_equal(got_split(ix, reads, 8, 4, 16, 4, MAIN, 0), want, nt.st, name)

    ix = FmIndex.from_text(nt.text, 0, 8, 0, nt.st, nt.hd).set_devices([0])
    for env in ("AWRY_ANCHOR_HIT_CAP=64", "AWRY_CHAIN_ALIGN_SUB_BATCH=7"):
        k, v = env.split("=")
        os.environ[k] = v
        try:
            check(ix, env)
        finally:
            del os.environ[k]
    before = L_.awry_debug_max_blocks()
    L_.awry_debug_set_max_blocks(2)
    try:
        check(ix, "a grid of two blocks")
    finally:
        L_.awry_debug_set_max_blocks(before)
    replicas = [0, 1] if torch.cuda.device_count() > 1 else [0, 0]
    for name, knob in (("two replicas", lambda: ix.set_devices(replicas)), ("k0", lambda: ix.set_seed_kmer_len(0)), ("k6", lambda: ix.set_seed_kmer_len(6))):
        knob()
        check(ix, name)
    ix.close()


def test_invalid_reads_and_an_amino_index_fail_as_the_siblings_do(nt):
    import awry_amd
    from awry_amd import _lib
    long_q = bytes(nt.text[100:1125])
    if b"$" in long_q or b"N" in long_q:
        long_q = b"ACGTTGCA" * 128 + b"A"
    assert len(long_q) == 1025
    for bad in (long_q, b"AC$T", b""):
        with pytest.raises(AwryError) as e:
            nt.ix.parallel_map_split_csr(*pack_queries([b"ACGT", b"GGA", bad, b"GGA"]), 1, 50)
        assert e.value.code == ERR_INVALID_QUERY and "query 2:" in str(e.value), bad[:8]
    L = awry_amd.load_library()
    u64p, u8p, u32p = C.POINTER(C.c_uint64), C.POINTER(C.c_uint8), C.POINTER(C.c_uint32)
    off, m, ps, coff, cg, st = u64p(), C.POINTER(_lib.MapSplit)(), C.POINTER(_lib.Pos)(), u64p(), u32p(), u8p()
    qb, qo = pack_queries([b"ACGT", long_q])
    rc = L.awry_map_split_batch(nt.ix._h, qb.ctypes.data, qo.ctypes.data_as(u64p), 2, 1, 50, 100, 16, 100, 10, 1, 4, 2, 1, 50, 4, 1, 4, 6, 5, 0, C.byref(off),
                                C.byref(m), C.byref(ps), C.byref(coff), C.byref(cg), C.byref(st))
    assert rc == ERR_INVALID_QUERY and not off and not m and not ps and not coff and not cg and not st
    t, st_, hd = synth.make_text(3_000, 1, 33, 1, 0.0)
    aa = FmIndex.from_text(t, 1, 8, 0, st_, hd).set_devices([0])
    try:
        with pytest.raises(AwryError) as e:
            aa.parallel_map_split_csr(*pack_queries([b"ACDEFGHIKLMNPQ"]))
        assert e.value.code == ERR_ARG
    finally:
        aa.close()
    src = nt.plants[0][0]
    assert nt.ix.map_split_string(bytes(nt.text[src:src + 101]), 12, 20)[0][3:] == (60, 0, "101=", 0, 101, 0, 101, 0)  # and the index still answers
