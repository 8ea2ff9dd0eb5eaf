"""Mapping on both strands on the GPU (awry_amd/csrc/kernels_map.hip.h, map_host.h) against tests/map_ref.py: the doubled batch of
awry_dev_revcomp at every length at which a group of lanes takes another step, awry_dev_map_select on the hand-made and on random
candidate lists in both passes, and awry_map_batch end to end -- against the reference, and against the composition that needs no
reference (awry_align_chains_batch on the doubled batch built on the host, ranked by map_ref's pure ranking function).  Everything
must be equal: offsets, records, positions, runs, status."""
import ctypes as C
import os

import numpy as np
import pytest

from awry_amd.fm_index import (ALN_DTYPE, CHAIN_DTYPE, ERR_ARG, ERR_INVALID_QUERY, MAP_DTYPE, MAP_SECONDARY, Q_SEED_CAP, AwryError, FmIndex, pack_queries)
from tests import chain_align_ref as ca
from tests import chain_ref as cr
from tests import map_ref as mp
from tests import mismatch_ref as mr
from tests import smem_ref as sr
from tests import synth
from tests.test_chain_align_gpu import KEY
from tests.test_chain_gpu import E2E_PARAMS, want_chains
from tests.test_map_cpu import FIXTURE, fixture_reads, hand_made_lists, placed_count
from tests.test_smems_gpu import World, edge_queries

pytestmark = pytest.mark.gpu

REVCOMP_LENGTHS = (1, 2, 63, 64, 65, 127, 128, 129, 1024)
SIZES = (1, 257, 3000)
AR = ((1, 1), (3, 1), (3, 6), (8, 16))
BANDS = (0, 4, 8)
P_MAIN = E2E_PARAMS[KEY]
P_SPECIAL = cr.Params(4, 16, 300, 20, 15)  # max_seeds = 4: the read from the repeat is abandoned on its forward strand


class OracleWorld(World):
    """tests/test_smems_gpu.py's World with the SMEMs of form (b), the oracle's counts: no string search, so the doubled batch of
    a few hundred reads takes seconds; the chains of a query are computed once per parameter set"""

    def __init__(self, *a):
        super().__init__(*a)
        self._chains = {}

    def ref(self, q):
        key = bytes(q)
        if key not in self._ref:
            self._ref[key] = sr.smems_oracle(self.oi, q, self.alphabet, 1)
        return self._ref[key]

    def chains_of(self, P):
        def get(qs):
            miss = [q for q in dict.fromkeys(bytes(q) for q in qs) if (q, P) not in self._chains]
            if miss:
                for q, c in zip(miss, want_chains(self, miss, *KEY, P)[0]):
                    self._chains[(q, P)] = c
            return [self._chains[(bytes(q), P)] for q in qs]
        return get


@pytest.fixture(scope="module")
def nt(oracle):
    return OracleWorld(oracle, *synth.make_text(40_000, 0, 21, 5, 0.03), 0)


def symbols(x):
    return [int(v) for v in mr.to_symbols(bytes(x), 0)]


# ---- awry_dev_revcomp ---------------------------------------------------------------------------------------------------------------

def revcomp_reads(n, seed):
    rng = np.random.default_rng(seed)
    letters = np.frombuffer(b"ACGTacgtUuNnRYKMSWBDHV$#\xe9\x00", np.uint8)
    out = []
    for i in range(n):
        L = REVCOMP_LENGTHS[i % len(REVCOMP_LENGTHS)] if n > 1 else 129
        weights = np.r_[np.full(4, 0.2), np.full(len(letters) - 4, 0.2 / (len(letters) - 4))]
        out.append(bytes(letters[rng.choice(len(letters), size=L, p=weights)]))
    if n > 4:
        out[3] = b""  # an empty read between the others: two empty queries
    return out


def revcomp_job(ix, reads, stream=None, lead=0):
    """upload (the offsets begin at `lead`, as a slice of a larger batch would), pre-fill the outputs with 0xEE, queue the launch"""
    qb, qo = pack_queries(reads)
    nb, n = len(qb), len(reads)
    j = dict(n=n, nb=nb, d_q=ix.dev_upload(np.concatenate([np.zeros(lead, np.uint8), qb, np.zeros(16, np.uint8)])), d_qo=ix.dev_upload(qo + np.uint64(lead)),
             d_ob=ix.dev_malloc(2 * nb + 32), d_oo=ix.dev_malloc(8 * (2 * n + 3)))
    ix.dev_memset(j["d_ob"], 0xEE, 2 * nb + 32)
    ix.dev_memset(j["d_oo"], 0xEE, 8 * (2 * n + 3))
    ix.dev_revcomp(j["d_q"], j["d_qo"], n, j["d_ob"], j["d_oo"], stream)
    return j


def assert_revcomp(ix, j, reads):
    ob = ix.dev_download(j["d_ob"], (2 * j["nb"] + 32,), np.uint8)
    oo = ix.dev_download(j["d_oo"], (2 * j["n"] + 3,), np.uint64)
    for key in ("d_q", "d_qo", "d_ob", "d_oo"):
        ix.dev_free(j[key])
    wb, wo = pack_queries(mp.doubled(reads))
    assert np.array_equal(oo[:2 * j["n"] + 1], wo) and np.all(oo[2 * j["n"] + 1:] == 0xEEEEEEEEEEEEEEEE)
    assert np.array_equal(ob[:2 * j["nb"]], wb) and np.all(ob[2 * j["nb"]:] == 0xEE)  # nothing written past the end


@pytest.mark.parametrize("n", SIZES)
def test_revcomp_equals_the_reference_at_every_length(nt, n):
    reads = revcomp_reads(n, 5 + n)
    assert n == 1 or {len(r) for r in reads} >= set(REVCOMP_LENGTHS) and any(b"$" in r for r in reads) and any(b"u" in r for r in reads)
    for lead in (0, 13):
        j = revcomp_job(nt.ix, reads, None, lead)
        nt.ix.dev_synchronize()
        assert_revcomp(nt.ix, j, reads)
    j = revcomp_job(nt.ix, [], None)  # no reads: one offset
    nt.ix.dev_synchronize()
    assert_revcomp(nt.ix, j, [])


def test_revcomp_on_two_streams_with_both_launches_queued_before_any_wait(nt):
    import torch
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    batches = [revcomp_reads(257, 1), revcomp_reads(3000, 2)]
    nt.ix.dev_synchronize()
    jobs = [revcomp_job(nt.ix, b, s.cuda_stream) for b, s in zip(batches, streams)]
    nt.ix.dev_synchronize()
    for j, b in zip(jobs, batches):
        assert_revcomp(nt.ix, j, b)


# ---- awry_dev_map_select ------------------------------------------------------------------------------------------------------------

def strand_lists(cands):
    """candidates (strand, j, edits, score, t_begin, t_end) -> per strand [(score, status, t_begin, t_end, edits)], the slots no
    candidate names filled with alignments that are not OK"""
    per = [[], []]
    for s, j, e, sc, tb, te in sorted(cands, key=lambda c: (c[0], c[1])):
        while len(per[s]) < j:
            per[s].append((999, ca.ALN_SKEW if len(per[s]) % 2 else ca.ALN_BAD_CHAIN, tb, te, 0))
        per[s].append((sc, ca.ALN_OK, tb, te, e))
    return per


def random_lists(n, seed, n_text):
    """per read (per-strand lists, capped): few distinct values per key, so that every key decides somewhere and spans collide"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        per = []
        for s in (0, 1):
            k = int(rng.choice([0, 0, 1, 1, 2, 3, 5, 8, 10]))
            lst = []
            for _ in range(k):
                tb = int(rng.choice([100, 150, 200, 5000, n_text - 120])) + int(rng.integers(0, 3))
                ln = int(rng.choice([0, 40, 60, 101]))
                st = ca.ALN_OK if rng.random() < 0.8 else int(rng.choice([ca.ALN_SKEW, ca.ALN_BAD_CHAIN]))
                lst.append((int(rng.choice([30, 60, 101])), st, tb, tb + ln, int(rng.integers(0, 4)) if st == ca.ALN_OK else 0))
            per.append(lst)
        out.append((per, bool(rng.random() < 0.1)))
    return out


def select_inputs(lists):
    n = len(lists)
    off, rows, status = [0], [], []
    for per, capped in lists:
        for s in (0, 1):
            rows += per[s]
            off.append(off[-1] + len(per[s]))
        status += [Q_SEED_CAP if capped else 0, 0]  # (the forward strand's byte carries it; either would do)
    alns, chains = np.zeros(max(1, len(rows)), ALN_DTYPE), np.zeros(max(1, len(rows)), CHAIN_DTYPE)
    for k, (sc, st, tb, te, e) in enumerate(rows):
        alns[k] = (tb, te, e, st)
        chains[k]["score"] = sc
    return np.array(off, np.uint64), alns, chains, np.array(status, np.uint8), n


def select_on_device(ix, inp, A, R):
    off, alns, chains, status, n = inp
    d = dict(off=ix.dev_upload(off), al=ix.dev_upload(alns.view(np.uint8)), ch=ix.dev_upload(chains.view(np.uint8)), st=ix.dev_upload(status),
             nm=ix.dev_malloc(8 * (n + 2)), rs=ix.dev_malloc(n + 8), mo=ix.dev_malloc(8 * (n + 1)), scr=ix.dev_malloc(ix.dev_scan_scratch_bytes(max(n, 1))))
    ix.dev_memset(d["nm"], 0xEE, 8 * (n + 2))
    ix.dev_memset(d["rs"], 0xEE, n + 8)
    ix.dev_map_select(d["off"], d["al"], d["ch"], d["st"], n, A, R, d["nm"], d["rs"])
    ix.dev_scan_counts(d["nm"], n, d["mo"], d["scr"])
    ix.dev_synchronize()
    nm, rs, mo = ix.dev_download(d["nm"], (n + 2,), np.uint64), ix.dev_download(d["rs"], (n + 8,), np.uint8), ix.dev_download(d["mo"], (n + 1,), np.uint64)
    tot = int(mo[-1])
    d.update(mp=ix.dev_malloc(32 * (tot + 2)), sel=ix.dev_malloc(4 * (tot + 2)), pos=ix.dev_malloc(16 * (tot + 2)))
    for key, size in (("mp", 32), ("sel", 4), ("pos", 16)):
        ix.dev_memset(d[key], 0xEE, size * (tot + 2))
    ix.dev_map_select(d["off"], d["al"], d["ch"], d["st"], n, A, R, None, None, d["mo"], d["mp"], d["sel"], d["pos"])
    ix.dev_synchronize()
    got = dict(nm=nm, rs=rs, mo=mo, mp=ix.dev_download(d["mp"], (32 * (tot + 2),), np.uint8), sel=ix.dev_download(d["sel"], (tot + 2,), np.uint32),
               pos=ix.dev_download(d["pos"], (tot + 2, 2), np.uint64))
    for p in d.values():
        ix.dev_free(p)
    return got


def positions_of(st, t_begin):
    starts = np.asarray(st, np.uint64)
    rec = np.searchsorted(starts, t_begin, side="right") - 1
    return np.stack([rec.astype(np.uint64), t_begin - starts[rec]], axis=1).reshape(-1, 2)


def assert_select(got, inp, A, R, st, what):
    off, alns, chains, status, n = inp
    woff, wrec, wsel, wst = mp.rank_alignments(off, chains, alns, status, n, A, R)
    tot = int(woff[-1])
    assert np.array_equal(got["mo"], woff), what
    assert np.array_equal(got["nm"][:n], np.diff(woff)) and np.all(got["nm"][n:] == 0xEEEEEEEEEEEEEEEE), what
    assert np.array_equal(got["rs"][:n], wst) and np.all(got["rs"][n:] == 0xEE), what
    g = got["mp"][:32 * tot].view(MAP_DTYPE)
    for f in MAP_DTYPE.names:
        bad = np.nonzero(g[f] != wrec[f])[0]
        assert not len(bad), (what, f, int(bad[0]), g[bad[0]], wrec[bad[0]])
    assert np.array_equal(got["sel"][:tot], np.array(wsel, np.uint32)), what
    assert np.array_equal(got["pos"][:tot], positions_of(st, wrec["t_begin"])), what
    assert np.all(got["mp"][32 * tot:] == 0xEE) and np.all(got["sel"][tot:] == 0xEEEEEEEE) and np.all(got["pos"][tot:] == 0xEEEEEEEEEEEEEEEE), what


@pytest.mark.parametrize("A", (1, 3, 8))
def test_map_select_equals_the_ranking_function_in_both_passes(nt, A):
    hand = [(strand_lists(c), capped) for _, c, capped, _ in hand_made_lists()]
    n_text = len(nt.text) - 1
    for n in SIZES:
        lists = (hand * (n // len(hand) + 1))[:n] if n <= len(hand) else hand + random_lists(n - len(hand), 100 + n, n_text)
        inp = select_inputs(lists)
        for R in range(1, 2 * A + 1) if n == 257 else sorted({1, A, 2 * A}):  # every R at one size, the ends and the middle at the others
            assert_select(select_on_device(nt.ix, inp, A, R), inp, A, R, nt.st, (A, R, n))
    inp = select_inputs(hand[1:2])  # one read, and no read
    assert_select(select_on_device(nt.ix, inp, A, 1), inp, A, 1, nt.st, (A, "one"))
    nt.ix.dev_map_select(None, None, None, None, 0, A, 1, None)


# ---- awry_map_batch -----------------------------------------------------------------------------------------------------------------

def want_maps(w, reads, A, R, W, P, memo):
    return mp.as_csr(mp.map_reads(w.tsym, reads, w.chains_of(P), A, R, W, memo))


def assert_maps_equal(got, want, st, what=None):
    off, maps, pos, coff, cg, status = got
    woff, wrec, wcoff, wcg, wst = want
    assert maps.dtype == MAP_DTYPE
    assert np.array_equal(off, woff) and np.array_equal(status, wst), what
    for f in MAP_DTYPE.names:
        bad = np.nonzero(maps[f] != wrec[f])[0]
        assert not len(bad), (what, f, int(bad[0]), maps[bad[0]], wrec[bad[0]])
    assert np.array_equal(pos, positions_of(st, wrec["t_begin"])), what
    assert np.array_equal(coff, wcoff) and np.array_equal(cg, wcg), what


def composition(ix, reads, A, R, W, P):
    """what needs no reference: awry_align_chains_batch on the doubled batch built on the host, ranked by the pure ranking function"""
    off, ch, al, coff, cg, st = ix.parallel_align_chains_csr(*pack_queries(mp.doubled(reads)), *KEY, A, W, *P)
    moff, rec, sel, rst = mp.rank_alignments(off, ch, al, st, len(reads), A, R)
    runs = [cg[int(coff[c]):int(coff[c + 1])] for c in sel]
    wcoff = np.zeros(len(sel) + 1, np.uint64)
    wcoff[1:] = np.cumsum([len(r) for r in runs], dtype=np.uint64)
    return moff, rec, wcoff, np.concatenate(runs + [np.zeros(0, np.uint32)]).astype(np.uint32), rst


@pytest.fixture(scope="module")
def main(nt):
    nt.tsym = symbols(nt.text)[:-1]
    fixture = fixture_reads(nt.text)
    reads = [r[0] for r in fixture] + [q for q in edge_queries(nt) if len(q) <= 1024]
    assert max(len(q) for q in reads) >= 1000
    return reads, fixture, {}


def special_text():
    """one record of random letters with, planted: a reverse palindrome; S, and elsewhere the reverse complement of S with two
    substitutions; a 40-letter unit six times between different flanks, and its reverse complement once"""
    rng = np.random.default_rng(404)
    rnd = lambda k: bytes(synth.NT[rng.integers(0, 4, size=k)])
    half = rnd(30)
    pal = half + mp.rc(half)
    S = rnd(60)
    S2 = bytearray(S)
    for at in (20, 41):
        S2[at] = b"ACGT"[(b"ACGT".index(S2[at]) + 1) % 4]
    U = rnd(40)
    body = rnd(500) + pal + rnd(400) + S + rnd(300) + mp.rc(bytes(S2)) + rnd(350)
    for _ in range(6):
        body += U + rnd(150)
    body += mp.rc(U) + rnd(200)
    absent = b"ACGT" * 8
    assert mp.rc(absent) == absent and all(absent[k:k + 12] not in body for k in range(4)) and body.count(U) == 6 and body.count(mp.rc(U)) == 1 and body.count(pal) == 1
    return np.frombuffer(body + b"$", np.uint8).copy(), dict(pal=pal, S=S, U=U, absent=absent, at_pal=500, at_S=960, at_U_rc=body.index(mp.rc(U)))


@pytest.fixture(scope="module")
def special(oracle):
    text, what = special_text()
    w = OracleWorld(oracle, text, [0], ["r0"], 0)
    w.tsym = symbols(text)[:-1]
    return w, what, [what["pal"], what["S"], what["absent"], what["U"], mp.rc(what["S"])], {}


def test_the_special_reads_hold_what_they_are_for(special):
    w, what, reads, memo = special
    per = mp.map_reads(w.tsym, reads, w.chains_of(P_SPECIAL), 3, 6, 4, memo)
    (st_pal, pal, _), (st_S, S, _), (st_no, none, _), (st_U, U, _), (_, rS, _) = per
    # the reverse palindrome: the same span on both strands, reported twice at R >= 2, MAPQ 0
    assert st_pal == 0 and [(r[0], r[1], r[2], r[5], r[6], r[7]) for r in pal] == [(500, 560, 0, 0, 0, 0), (500, 560, 0, 1, 0, MAP_SECONDARY)]
    # both strands occur, at different edit counts: 0 edits forward, 2 on the reverse strand -> MAPQ 20
    assert st_S == 0 and [(r[0], r[2], r[5], r[6]) for r in S] == [(960, 0, 0, 20), (960 + 60 + 300, 2, 1, 0)]
    assert [(r[2], r[5]) for r in rS] == [(0, 1), (2, 0)] and rS[0][6] == 20  # and the read given on the other strand mirrors it
    assert (st_no, none) == (0, [])  # no seed: no record, no error
    # six seeds forward > max_seeds = 4: that strand is abandoned, the read's status says so, the reverse strand's hit has MAPQ 0
    assert st_U == Q_SEED_CAP and [(r[0], r[2], r[5], r[6]) for r in U] == [(what["at_U_rc"], 0, 1, 0)]


@pytest.mark.parametrize("band", BANDS)
def test_batch_equals_the_reference_and_the_composition(nt, main, special, band):
    reads, fixture, memo = main
    for A, R in AR:
        want = want_maps(nt, reads, A, R, band, P_MAIN, memo)
        got = nt.ix.parallel_map_csr(*pack_queries(reads), *KEY, A, R, band, *P_MAIN)
        assert_maps_equal(got, want, nt.st, (A, R, band))
        assert_maps_equal(got, composition(nt.ix, reads, A, R, band, P_MAIN), nt.st, ("composition", A, R, band))
        assert int(got[0][-1]) > len(reads) // 2
        if (A, R, band) == (3, 1, 4):
            per = mp.map_reads(nt.tsym, [r[0] for r in fixture], nt.chains_of(P_MAIN), 4, 1, 4, memo)
            assert placed_count(fixture, per) == FIXTURE["placed"] >= FIXTURE["placed_min"]  # the fixture's character, as the CPU suite records it
    w, _, sreads, smemo = special
    for A, R in AR:
        want = want_maps(w, sreads, A, R, band, P_SPECIAL, smemo)
        got = w.ix.parallel_map_csr(*pack_queries(sreads), *KEY, A, R, band, *P_SPECIAL)
        assert_maps_equal(got, want, w.st, ("special", A, R, band))
        assert_maps_equal(got, composition(w.ix, sreads, A, R, band, P_SPECIAL), w.st, ("special composition", A, R, band))


def test_the_list_api_and_the_call_without_the_optional_arrays(nt, main):
    reads, _, memo = main
    woff, wrec, wcoff, wcg, _ = want_maps(nt, reads[:4], 3, 6, 4, P_MAIN, memo)
    pos = positions_of(nt.st, wrec["t_begin"])
    from awry_amd.fm_index import cigar_string
    want = [[(int(pos[c][0]), int(pos[c][1]), int(wrec[c]["strand"]), int(wrec[c]["mapq"]), int(wrec[c]["edits"]),
              cigar_string(wcg[int(wcoff[c]):int(wcoff[c + 1])]), int(wrec[c]["flags"])) for c in range(int(woff[i]), int(woff[i + 1]))] for i in range(4)]
    assert nt.ix.parallel_map(reads[:4], *KEY, 3, 6, 4, **P_MAIN._asdict()) == want and sum(len(x) for x in want) >= 4
    assert nt.ix.map_string(reads[1], *KEY, 3, 6, 4, **P_MAIN._asdict()) == want[1] and want[1][0][2] == 1  # the second fixture read is reversed
    qb, qo = pack_queries(reads)
    full = nt.ix.parallel_map_csr(qb, qo, *KEY, 3, 6, 4, *P_MAIN)
    bare = nt.ix.parallel_map_csr(qb, qo, *KEY, 3, 6, 4, *P_MAIN, want_pos=False, want_cigar=False)
    assert np.array_equal(bare[0], full[0]) and np.array_equal(bare[1], full[1]) and np.array_equal(bare[5], full[5])
    assert len(bare[2]) == 0 and len(bare[3]) == 0 and len(bare[4]) == 0
    nopos = nt.ix.parallel_map_csr(qb, qo, *KEY, 3, 6, 4, *P_MAIN, want_pos=False)
    assert np.array_equal(nopos[3], full[3]) and np.array_equal(nopos[4], full[4]) and len(nopos[2]) == 0


@pytest.mark.parametrize("n", SIZES)
def test_batch_sizes(nt, main, n):
    reads, _, memo = main
    short = [q for q in reads if len(q) <= 260]
    sub = [short[(7 * i) % len(short)] for i in range(n)]
    want = want_maps(nt, sub, 3, 6, 4, P_MAIN, memo)
    assert_maps_equal(nt.ix.parallel_map_csr(*pack_queries(sub), *KEY, 3, 6, 4, *P_MAIN), want, nt.st, n)


def test_results_do_not_depend_on_capacity_sub_batch_replicas_table_or_accelerators(nt, main):
    import awry_amd
    reads, _, memo = main
    qb, qo = pack_queries(reads)
    text, st = nt.text, nt.st
    hd = ["r%d" % i for i in range(len(st))]
    want = want_maps(nt, reads, 3, 6, 4, P_MAIN, memo)

    def check(ix, name):
        assert_maps_equal(ix.parallel_map_csr(qb, qo, *KEY, 3, 6, 4, *P_MAIN), want, st, name)

    ix = FmIndex.from_text(text, 0, 8, 0, st, hd).set_devices([0])
    for env in ("AWRY_ANCHOR_HIT_CAP=64", "AWRY_CHAIN_ALIGN_SUB_BATCH=7"):  # 64 hits: the halving fallback, down to single reads
        k, v = env.split("=")
        os.environ[k] = v
        try:
            check(ix, env)
        finally:
            del os.environ[k]
    for name, knob in (("two replicas", lambda: ix.set_devices([0, 0])), ("k0", lambda: ix.set_seed_kmer_len(0)), ("k6", lambda: ix.set_seed_kmer_len(6)),
                       ("verify off", lambda: ix.set_verify(-1)), ("lcx off", lambda: ix.set_lcx(False)), ("dense sa", lambda: ix.set_locate_sa_ratio(1))):
        knob()
        check(ix, name)
    ix.close()
    L_ = awry_amd.load_library()
    L_.awry_debug_force_wide_rows(1)
    try:
        wide = FmIndex.from_text(text, 0, 8, 0, st, hd).set_devices([0])
    finally:
        L_.awry_debug_force_wide_rows(0)
    try:
        assert "wide" in wide.count_schedule(31)
        with pytest.raises(AwryError) as e:
            wide.parallel_map_csr(qb, qo, *KEY, 3, 6, 4, *P_MAIN)
        assert e.value.code == ERR_ARG
    finally:
        wide.close()


def test_invalid_reads_fail_the_batch_and_name_the_read(nt):
    import awry_amd
    from awry_amd import _lib
    long_q = bytes(nt.text[100:1125])
    assert len(long_q) == 1025 and b"$" not in long_q
    for bad in (long_q, b"AC$T", b""):
        with pytest.raises(AwryError) as e:
            nt.ix.parallel_map_csr(*pack_queries([b"ACGT", b"GGA", bad, b"GGA"]), 1, 50)
        assert e.value.code == ERR_INVALID_QUERY and "query 2:" in str(e.value), bad[:8]  # the read's own index, not one into the doubled batch
    L = awry_amd.load_library()
    u64p, u8p, u32p = C.POINTER(C.c_uint64), C.POINTER(C.c_uint8), C.POINTER(C.c_uint32)
    for bad in (long_q, b"AC$T"):
        off, m, ps, coff, cg, st = u64p(), C.POINTER(_lib.Map)(), C.POINTER(_lib.Pos)(), u64p(), u32p(), u8p()
        qb, qo = pack_queries([b"ACGT", bad])
        rc = L.awry_map_batch(nt.ix._h, qb.ctypes.data, qo.ctypes.data_as(u64p), 2, 1, 50, 100, 16, 100, 10, 1, 4, 1, 4, C.byref(off), C.byref(m),
                              C.byref(ps), C.byref(coff), C.byref(cg), C.byref(st))
        assert rc == ERR_INVALID_QUERY and not off and not m and not ps and not coff and not cg and not st
    t, st_, hd = synth.make_text(3_000, 1, 33, 1, 0.0)
    aa = FmIndex.from_text(t, 1, 8, 0, st_, hd).set_devices([0])
    with pytest.raises(AwryError) as e:
        aa.parallel_map_csr(*pack_queries([b"ACDEFGHIKLMNPQ"]))
    assert e.value.code == ERR_ARG
    aa.close()
    got = nt.ix.map_string(bytes(nt.text[100:1124]), 12, 20)  # and the index still answers: a 1024-letter read, and its reverse complement
    assert got == [(0, 100, 0, 60, 0, "1024=", 0)] and nt.ix.map_string(mp.rc(nt.text[100:1124]), 12, 20) == [(0, 100, 1, 60, 0, "1024=", 0)]


# ---- the chunk driver's rarely taken branches, on 64 reads of 101 letters ------------------------------------------------------------

from tests.test_smems_gpu import all_equal, shrunk_cap, small_reads, with_bad_read  # noqa: E402

NO_CHAIN = P_MAIN._replace(min_score=10 ** 6)  # above any reachable score


def assert_no_records(got, n):
    off, maps, pos, coff, cg, st = got
    assert np.array_equal(off, np.zeros(n + 1, np.uint64)) and len(maps) == 0 and len(pos) == 0 and np.array_equal(coff, [0]) and len(cg) == 0
    assert st.dtype == np.uint8 and np.array_equal(st, np.zeros(n, np.uint8))


def test_chunks_without_smems_and_without_chains_give_zero_offsets_and_ok_status(nt):
    reads = small_reads(nt)
    qb, qo = pack_queries(reads)
    assert_no_records(nt.ix.parallel_map_csr(qb, qo, 102, 20, 3, 6, 4, *P_MAIN), len(reads))  # min_len above every read's length: no candidate
    assert int(nt.ix.parallel_locate_smems_csr(qb, qo, KEY[1], KEY[0])[2][-1]) >= len(reads)  # seeds, and no chain of them
    assert_no_records(nt.ix.parallel_map_csr(qb, qo, *KEY, 3, 6, 4, *NO_CHAIN), len(reads))


def test_a_bad_read_is_named_under_its_own_index_before_the_capacity_test_splits_its_chunk(nt):
    reads = small_reads(nt, 6)
    # '#' is '$' on the reverse strand; the non-ASCII byte is 'N' there, so only the read as given is rejected -- under the read's index
    for bad, why in ((b"AC$T", "'$' or '#'"), (b"", "empty query"), (b"AC#T", "'$' or '#'"), (bytes([0x41, 0x80, 0x43]), "non-ASCII")):
        with shrunk_cap("AWRY_ANCHOR_HIT_CAP"):
            with pytest.raises(AwryError) as e:
                nt.ix.parallel_map_csr(*pack_queries(with_bad_read(reads, bad)), *KEY, 3, 6, 4, *P_MAIN)
        print(bad, str(e.value))
        assert e.value.code == ERR_INVALID_QUERY and "query 3: " in str(e.value) and why in str(e.value), bad


def test_seven_reads_halved_down_to_single_reads_equal_the_uncapped_call(nt):
    qb, qo = pack_queries(small_reads(nt, 7))
    want = nt.ix.parallel_map_csr(qb, qo, *KEY, 3, 6, 4, *P_MAIN)
    assert int(want[0][-1]) >= 7
    with shrunk_cap("AWRY_ANCHOR_HIT_CAP"):
        assert all_equal(want, nt.ix.parallel_map_csr(qb, qo, *KEY, 3, 6, 4, *P_MAIN))
