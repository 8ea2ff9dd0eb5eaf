"""Chaining on the GPU (awry_amd/csrc/kernels_chain.hip.h) against tests/chain_ref.py: the device primitive on synthetic seeds --
every size at which the kernel takes another path, ties of every key, both lane-group widths, streams, the census -- and the
batch entry point end to end with seeds from tests/smem_ref.py and the oracle's locate lists.  Everything must be equal:
offsets, records, members, status."""
import os

import numpy as np
import pytest

from awry_amd.fm_index import CHAIN_DTYPE, ERR_INVALID_QUERY, Q_SEED_CAP, SEED_DTYPE, AwryError, FmIndex, pack_queries
from tests import chain_ref as cr
from tests import smem_ref as sr
from tests import synth
from tests.test_anchors_gpu import nt_queries, planted
from tests.test_smems_gpu import World, edge_queries, nfree_world

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 2, 3, 15, 16, 17, 18, 63, 64, 65, 300, 4096]  # the tile of the 16-lane groups is 64 seeds, of the waves 256
LOOKBACKS = [1, 2, 16, 17, 64]
E2E_PARAMS = {(1, 50): cr.Params(2000, 32, 300, 20, 15), (12, 20): cr.Params(2000, 16, 300, 20, 15)}
# what tests/chain_ref.py gives (computed on the CPU when the test was written):
#   the 200 planted reads at (min_len, max_hits) = (12, 20): primaries within the planted indel total of the origin's diagonal 200 of
#   200 (the condition is 95 %: 190), primaries of >= 2 seeds 173 (the condition is more than half)
#   the tandem-repeat query at (4, 200): 177 seeds, 100 chains
FIXTURE = dict(placed_min=190, placed=200, multi_seed_min=101, multi_seed=173, tandem_seeds=177, tandem_chains=100)


@pytest.fixture(scope="module")
def nt(oracle):
    return World(oracle, *synth.make_text(40_000, 0, 21, 5, 0.03), 0)


# ---- the device primitive on synthetic seeds -----------------------------------------------------------------------------------

def synthetic_sets(st):
    """seed sets of the SIZES and special sets; coordinates lie around the join of records 1 and 2 (st[2])"""
    rng = np.random.default_rng(77)
    join = int(st[2])
    sets = []
    for n in SIZES:
        span = max(40, 3 * n // 2)
        diags = [join - span // 2, join - span // 2 + 7, join + 11]
        seeds = []
        for _ in range(n):
            q = int(rng.integers(0, span))
            if rng.random() < 0.7:
                t = diags[int(rng.integers(0, 3))] + q + int(rng.integers(-2, 3))
            else:
                t = join - span + int(rng.integers(0, 2 * span))
            seeds.append((q, int(rng.choice([1, 3, 8, 21])), t))
        sets.append(seeds)
    base = join - 5000
    sets += [
        [(5, 10, base + 5)] * 4 + [(20, 10, base + 20)] * 3 + [(5, 9, base + 5), (5, 11, base + 5)],       # duplicates of (t_pos, q_begin) and of whole seeds
        [(0, 10, base), (2, 10, base), (13, 5, base + 12), (30, 5, base + 31)],                            # equal candidates (skew 1 either way): the largest j wins
        [(0, 10, base), (100, 10, base + 300), (200, 10, base + 600), (10, 4, base + 10), (110, 4, base + 310)],  # equal f: the visit order breaks the tie
        [(0, 30, base), (1, 3, base + 6), (2, 3, base + 12), (40, 30, base + 41)],                         # negative gains (skew above the seed length)
        [(0, 10, join - 30), (15, 10, join - 15), (30, 10, join), (45, 10, join + 15)],                    # a diagonal across the record join
        [(0, 10, base), (20, 10, base + 20), (40, 10, base + 40), (60, 10, base + 60), (80, 10, base + 80), (45, 12, base + 51), (65, 12, base + 71),
         (85, 12, base + 91)],                                                                            # a fork: the second branch is a truncated chain
        [(int(rng.integers(0, 3000)), 5, base + int(rng.integers(0, 3000))) for _ in range(4097)],        # one seed over max_seeds = 4096
        [(3, 4, base + 3)],
    ]
    return sets


def reference(sets, st, P):
    per = [cr.chain_query(s, [int(x) for x in st], P) for s in sets]
    return cr.as_csr([(a, b) for a, b, _ in per]), tuple(sum(t[k] for _, _, t in per) for k in range(3))


def device_job(ix, sets, P, stream=None, tally=False):
    """upload, pre-fill the outputs with 0xEE; run() queues count, two scans and fill on the stream; result() downloads"""
    n = len(sets)
    soff = np.zeros(n + 1, np.uint64)
    soff[1:] = np.cumsum([len(s) for s in sets], dtype=np.uint64)
    flat = np.zeros(max(1, int(soff[-1])), SEED_DTYPE)
    rows = [x for s in sets for x in s]
    if rows:
        a = np.array(rows, np.int64)
        flat["q_begin"], flat["q_len"], flat["t_pos"] = a[:, 0], a[:, 1], a[:, 2]
    cap_c, cap_m = int(soff[-1]) + 4, int(soff[-1]) + 4
    j = dict(n=n, s=stream, P=P, cap_c=cap_c, cap_m=cap_m, tally=tally, d_so=ix.dev_upload(soff), d_sd=ix.dev_upload(flat.view(np.uint8)),
             d_nc=ix.dev_malloc(8 * n), d_nm=ix.dev_malloc(8 * n), d_co=ix.dev_malloc(8 * (n + 1)), d_mo=ix.dev_malloc(8 * (n + 1)),
             d_scr=ix.dev_malloc(ix.dev_scan_scratch_bytes(n)), d_st=ix.dev_malloc(n), d_c=ix.dev_malloc(32 * cap_c), d_m=ix.dev_malloc(16 * cap_m),
             d_t=ix.dev_malloc(24))
    ix.dev_memset(j["d_c"], 0xEE, 32 * cap_c)
    ix.dev_memset(j["d_m"], 0xEE, 16 * cap_m)
    ix.dev_memset(j["d_st"], 0xEE, n)
    ix.dev_memset(j["d_t"], 0, 24)
    return j


def run_job(ix, j):
    P, s, n = j["P"], j["s"], j["n"]
    if j["tally"]:
        ix.dev_chain_seeds_tally(j["d_so"], j["d_sd"], n, *P, j["d_nc"], j["d_nm"], j["d_t"], None, None, None, None, j["d_st"], s)
    else:
        ix.dev_chain_seeds(j["d_so"], j["d_sd"], n, *P, j["d_nc"], j["d_nm"], None, None, None, None, j["d_st"], s)
    ix.dev_scan_counts(j["d_nc"], n, j["d_co"], j["d_scr"], s)
    ix.dev_scan_counts(j["d_nm"], n, j["d_mo"], j["d_scr"], s)
    ix.dev_chain_seeds(j["d_so"], j["d_sd"], n, *P, None, None, j["d_co"], j["d_mo"], j["d_c"], j["d_m"], None, s)


def job_result(ix, j):
    n = j["n"]
    out = dict(nc=ix.dev_download(j["d_nc"], (n,), np.uint64), nm=ix.dev_download(j["d_nm"], (n,), np.uint64),
               co=ix.dev_download(j["d_co"], (n + 1,), np.uint64), mo=ix.dev_download(j["d_mo"], (n + 1,), np.uint64),
               st=ix.dev_download(j["d_st"], (n,), np.uint8), c=ix.dev_download(j["d_c"], (32 * j["cap_c"],), np.uint8),
               m=ix.dev_download(j["d_m"], (16 * j["cap_m"],), np.uint8), t=ix.dev_download(j["d_t"], (3,), np.uint64))
    for key in ("d_so", "d_sd", "d_nc", "d_nm", "d_co", "d_mo", "d_scr", "d_st", "d_c", "d_m", "d_t"):
        ix.dev_free(j[key])
    return out


def assert_equals_reference(got, want, cap_c, cap_m):
    (woff, wrows, wsoff, wmem, wst) = want
    assert np.array_equal(got["st"], wst)
    assert np.array_equal(got["nc"], np.diff(woff)) and np.array_equal(got["co"], woff)
    tot, mem = int(woff[-1]), int(wsoff[-1])
    per_query_members = np.array([int(wsoff[int(woff[q + 1])] - wsoff[int(woff[q])]) for q in range(len(woff) - 1)], np.uint64)
    assert np.array_equal(got["nm"], per_query_members) and np.array_equal(got["mo"][1:], np.cumsum(per_query_members, dtype=np.uint64))
    chains = got["c"][:32 * tot].view(CHAIN_DTYPE)
    assert np.array_equal(cr.got_chain_rows(chains), wrows)
    assert np.array_equal(cr.got_seed_rows(got["m"][:16 * mem].view(SEED_DTYPE)), wmem)
    assert np.all(got["c"][32 * tot:] == 0xEE) and np.all(got["m"][16 * mem:] == 0xEE)  # nothing written past the last record


@pytest.fixture(scope="module")
def synthetic(nt):
    sets = synthetic_sets(nt.st)
    return sets, {lb: reference(sets, nt.st, cr.Params(4096, lb, 120, 6, 4)) for lb in LOOKBACKS}


def test_the_synthetic_sets_hold_what_they_are_for(nt, synthetic):
    sets, refs = synthetic
    st = [int(x) for x in nt.st]
    assert [len(s) for s in sets[:len(SIZES)]] == SIZES and all(lb in SIZES and lb + 1 in SIZES for lb in LOOKBACKS)
    P = cr.Params(4096, 16, 120, 6, 4)
    dup, eqc, eqf, neg, joinset, inter, over, _ = sets[len(SIZES):]
    assert len(set(dup)) < len(dup)
    s = cr.sort_seeds(eqc)
    f, p, _ = cr.scores(s, [0] * 4, P)
    cands = [f[j] + cr.gain(s[j], s[2]) for j in (0, 1)]
    assert cands[0] == cands[1] > s[2][1] and p[2] == 1  # equal candidates: the largest j
    s = cr.sort_seeds(eqf)
    f, _, _ = cr.scores(s, [0] * 5, P)
    assert len(set(f)) < len(f)
    s = cr.sort_seeds(neg)
    assert any(cr.admissible(s[j], s[i], 0, 0, P) and cr.gain(s[j], s[i]) < 0 for i in range(4) for j in range(i))
    chains = cr.chain_query(joinset, st, P)[1]
    assert all({cr.record_of(st, m[2]) for m in c[6]} in ({1}, {2}) for c in chains) and len(chains) == 2  # never chained across the join
    assert len(cr.chain_query(joinset, [0], P)[1]) == 1                                                   # (one record: one chain)
    assert any(b > 0 for b in cr.chain_bases(inter, st, P))  # a truncated chain
    assert any(b > 0 for seeds in sets[:len(SIZES)] for b in cr.chain_bases(seeds, st, P))
    assert len(over) == 4097
    for lb in LOOKBACKS:
        wst = refs[lb][0][4]
        assert [int(x) for x in np.nonzero(wst)[0]] == [len(SIZES) + 6] and wst[len(SIZES) + 6] == Q_SEED_CAP
        assert int(np.diff(refs[lb][0][0])[len(SIZES) + 7]) == 1 and int(np.diff(refs[lb][0][0])[len(SIZES) - 1]) > 1  # the neighbours have chains


@pytest.mark.parametrize("lookback", LOOKBACKS)
def test_device_primitive_equals_the_reference_in_both_group_widths(nt, synthetic, lookback):
    sets, refs = synthetic
    want, wtally = refs[lookback]
    P = cr.Params(4096, lookback, 120, 6, 4)
    results = []
    for width in ((None, "64") if lookback <= 16 else (None,)):
        if width:
            os.environ["AWRY_CHAIN_GROUP"] = width
        try:
            j = device_job(nt.ix, sets, P, tally=True)
            run_job(nt.ix, j)
            nt.ix.dev_synchronize()
        finally:
            os.environ.pop("AWRY_CHAIN_GROUP", None)
        got = job_result(nt.ix, j)
        assert_equals_reference(got, want, j["cap_c"], j["cap_m"])
        assert tuple(int(x) for x in got["t"]) == wtally  # seeds chained, pairs evaluated, chains reported (the count pass)
        results.append(got)
    for other in results[1:]:
        assert all(np.array_equal(results[0][k], other[k]) for k in results[0])


def test_max_skew_zero_and_small_caps(nt, synthetic):
    sets, _ = synthetic
    sets = sets[:len(SIZES) - 1] + sets[len(SIZES):len(SIZES) + 6]
    for P in (cr.Params(64, 16, 50, 0, 1), cr.Params(17, 64, 3, 1, 2), cr.Params(299, 3, 4000, 4000, 8)):
        want, wtally = reference(sets, nt.st, P)
        assert want[4].any() and not want[4].all() and int(want[0][-1]) > 10
        j = device_job(nt.ix, sets, P, tally=True)
        run_job(nt.ix, j)
        nt.ix.dev_synchronize()
        got = job_result(nt.ix, j)
        assert_equals_reference(got, want, j["cap_c"], j["cap_m"])
        assert tuple(int(x) for x in got["t"]) == wtally


def test_two_streams_with_all_launches_queued_before_any_wait(nt, synthetic):
    import torch
    sets, refs = synthetic
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    plan = [(sets, 16), (sets[::-1], 64)]
    jobs = [device_job(nt.ix, s, cr.Params(4096, lb, 120, 6, 4), stream=st.cuda_stream) for (s, lb), st in zip(plan, streams)]
    nt.ix.dev_synchronize()
    for j in jobs:
        run_job(nt.ix, j)
    nt.ix.dev_synchronize()
    assert_equals_reference(job_result(nt.ix, jobs[0]), refs[16][0], jobs[0]["cap_c"], jobs[0]["cap_m"])
    assert_equals_reference(job_result(nt.ix, jobs[1]), reference(sets[::-1], nt.st, cr.Params(4096, 64, 120, 6, 4))[0], jobs[1]["cap_c"], jobs[1]["cap_m"])


# ---- end to end -------------------------------------------------------------------------------------------------------------------

def planted_with_indels(text, rng):
    """-> (read, origin, indel total): 101..250 letters of the text with 0..5 substitutions and 0..2 indels of 1..3 letters"""
    L = int(rng.integers(101, 251))
    p = int(rng.integers(0, len(text) - 1 - L - 8))
    q = bytearray(planted(text[p:p + L + 2], np.random.default_rng(int(rng.integers(0, 1 << 30))), L, int(rng.integers(0, 6)), synth.NT))
    total = 0
    for _ in range(int(rng.integers(0, 3))):
        at, k = int(rng.integers(20, len(q) - 20)), int(rng.integers(1, 4))
        if rng.random() < 0.5:
            del q[at:at + k]
        else:
            q[at:at] = bytes(synth.NT[rng.integers(0, 4, size=k)])
        total += k
    return bytes(q), p, total


def indel_reads(text, n=200, seed=31):
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        q, p, total = planted_with_indels(text, rng)
        if b"N" not in q:  # (a read across a record join or an N run has no single origin)
            out.append((q, p, total))
    return out


def want_chains(w, qs, min_len, max_hits, P):
    per = [[a for a in w.ref(q) if a[1] >= min_len] for q in qs]
    seeds = cr.seeds_from_smems(w.oi, qs, per, w.alphabet, max_hits)
    st = [int(x) for x in w.st]
    return [cr.chain_query(s, st, P)[:2] for s in seeds], seeds


def assert_batch_equals(got, want_per):
    off, ch, soff, sd, st = got
    woff, wrows, wsoff, wmem, wst = cr.as_csr(want_per)
    assert ch.dtype == CHAIN_DTYPE and sd.dtype == SEED_DTYPE
    assert np.array_equal(off, woff) and np.array_equal(st, wst)
    assert np.array_equal(cr.got_chain_rows(ch), wrows)
    assert np.array_equal(soff, wsoff) and np.array_equal(cr.got_seed_rows(sd), wmem)


@pytest.fixture(scope="module")
def e2e(nt):
    reads = indel_reads(nt.text)
    qs = [q for q in nt_queries(nt, (6, nt.ix.seed_kmer_len())) + edge_queries(nt)] + [q for q, _, _ in reads]
    want = {key: want_chains(nt, qs, *key, P) for key, P in E2E_PARAMS.items()}
    return qs, reads, want


def test_batch_equals_the_reference_and_the_fixture_has_its_character(nt, e2e):
    qs, reads, want = e2e
    qb, qo = pack_queries(qs)
    for key, P in E2E_PARAMS.items():
        got = nt.ix.parallel_chains_csr(qb, qo, *key, *P)
        assert_batch_equals(got, want[key][0])
        assert int(got[0][-1]) > len(qs) // 2
    # the character of the fixture, from the reference: the planted reads are placed, and mostly by chains of several seeds
    per = want[(12, 20)][0][-len(reads):]
    placed = sum(1 for (st, chains), (_, p, total) in zip(per, reads) if chains and abs(chains[0][4] - chains[0][2] - p) <= total)
    multi = sum(1 for st, chains in per if chains and chains[0][1] >= 2)
    print("planted reads placed by the primary chain: %d of %d; primaries of >= 2 seeds: %d" % (placed, len(reads), multi))
    assert placed >= FIXTURE["placed_min"] and placed == FIXTURE["placed"] and multi >= FIXTURE["multi_seed_min"] and multi == FIXTURE["multi_seed"]
    assert any(st == Q_SEED_CAP for st, _ in want[(1, 50)][0]) or max(len(s) for s in want[(1, 50)][1]) <= 2000
    # the list API
    i = len(qs) - 3
    lst = nt.ix.parallel_chains(qs[i:i + 2], 12, 20, **E2E_PARAMS[(12, 20)]._asdict())
    assert lst == [[(c[0], c[2], c[3], c[4], c[5], c[6]) for c in chains] for _, chains in want[(12, 20)][0][i:i + 2]]
    assert nt.ix.chains_string(qs[i], 12, 20, **E2E_PARAMS[(12, 20)]._asdict()) == lst[0]
    nos = nt.ix.parallel_chains_csr(qb, qo, 12, 20, *E2E_PARAMS[(12, 20)], want_seeds=False)
    assert np.array_equal(nos[1], nt.ix.parallel_chains_csr(qb, qo, 12, 20, *E2E_PARAMS[(12, 20)])[1]) and len(nos[3]) == 0


@pytest.mark.parametrize("n", [1, 257, 3000])
def test_batch_sizes(nt, e2e, n):
    qs, _, want = e2e
    short = [i for i, q in enumerate(qs) if len(q) <= 260]
    pick = [short[(7 * i) % len(short)] for i in range(n)]
    for key, P in E2E_PARAMS.items():
        assert_batch_equals(nt.ix.parallel_chains_csr(*pack_queries([qs[i] for i in pick]), *key, *P), [want[key][0][i] for i in pick])


def test_results_do_not_depend_on_capacity_replicas_table_accelerators_or_row_width(nt, e2e):
    import awry_amd
    qs, _, want = e2e
    qb, qo = pack_queries(qs)
    text, st = nt.text, nt.st
    hd = ["r%d" % i for i in range(len(st))]

    def check(ix, name):
        for key, P in E2E_PARAMS.items():
            try:
                assert_batch_equals(ix.parallel_chains_csr(qb, qo, *key, *P), want[key][0])
            except AssertionError as e:
                raise AssertionError("%s %s" % (name, key)) from e

    ix = FmIndex.from_text(text, 0, 8, 0, st, hd).set_devices([0])
    os.environ["AWRY_ANCHOR_HIT_CAP"] = "64"  # chunks split until each fits (or holds one query)
    try:
        check(ix, "hit cap 64")
    finally:
        del os.environ["AWRY_ANCHOR_HIT_CAP"]
    for name, knob in (("k0", lambda: ix.set_seed_kmer_len(0)), ("k6", lambda: ix.set_seed_kmer_len(6)), ("verify off", lambda: ix.set_verify(-1)),
                       ("lcx off", lambda: ix.set_lcx(False)), ("dense sa", lambda: ix.set_locate_sa_ratio(1)), ("two replicas", lambda: ix.set_devices([0, 0]))):
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
        check(wide, "wide rows")
    finally:
        wide.close()


def test_invalid_query_in_a_batch_is_rejected_and_out_pointers_stay(nt):
    import ctypes as C
    import awry_amd
    from awry_amd import _lib
    for bad in (b"AC$T", b"", b"A#", bytes([0x41, 0x80])):
        qb, qo = pack_queries([b"ACGT", bad, b"GGA"])
        with pytest.raises(AwryError) as e:
            nt.ix.parallel_chains_csr(qb, qo, 1, 50)
        assert e.value.code == ERR_INVALID_QUERY, bad
    L = awry_amd.load_library()
    u64p, u8p = C.POINTER(C.c_uint64), C.POINTER(C.c_uint8)
    off, ch, soff, sd, st = u64p(), C.POINTER(_lib.Chain)(), u64p(), C.POINTER(_lib.Seed)(), u8p()
    qb, qo = pack_queries([b"ACGT", b"AC$T"])
    rc = L.awry_chain_batch(nt.ix._h, qb.ctypes.data, qo.ctypes.data_as(u64p), 2, 1, 50, 100, 16, 100, 10, 1, C.byref(off), C.byref(ch), C.byref(soff),
                            C.byref(sd), C.byref(st))
    assert rc == ERR_INVALID_QUERY and not off and not ch and not soff and not sd and not st
    assert nt.ix.chains_string(b"ACGT", 1, 50, min_score=1) is not None  # and the index still answers


TANDEM_QUERY = b"ACGT" * 15 + b"TT" + b"ACGT" * 15  # two SMEMs, each at every begin of the array in phase with it


def tandem_world_and_query(oracle):
    rng = np.random.default_rng(12)
    flank = lambda: bytes(synth.NT[rng.integers(0, 4, size=300)])
    return nfree_world(oracle, flank() + b"ACGT" * 100 + flank()), TANDEM_QUERY


def test_tandem_repeat_gives_many_seeds_and_several_chains(oracle):
    w, q = tandem_world_and_query(oracle)
    P = cr.Params(4096, 64, 500, 50, 10)
    want, seeds = want_chains(w, [q], 4, 200, P)
    print("tandem query: %d seeds, %d chains" % (len(seeds[0]), len(want[0][1])))
    assert len(seeds[0]) == FIXTURE["tandem_seeds"] > 64 and len(want[0][1]) == FIXTURE["tandem_chains"] > 1
    assert_batch_equals(w.ix.parallel_chains_csr(*pack_queries([q]), 4, 200, *P), want)
    w.ix.close()


def test_oracle_scale_seeds_on_a_2_mbp_text(oracle):
    text, st, hd = synth.make_text(2_000_000, 0, 24, 6, 0.01)
    ix = FmIndex.from_text(text, 0, 8, 0, st, hd).set_devices([0])
    oi = oracle.OracleIndex.from_text(text, 0, 8, 0, st, hd)
    rng = np.random.default_rng(5)
    qs = [planted(text, rng, 101, int(rng.integers(0, 4)), synth.NT) for _ in range(400)] + [bytes(q) for q in synth.random_queries(50, 101, 0, 6)]
    P = cr.Params(500, 16, 200, 10, 12)
    per = [sr.smems_oracle(oi, q, 0, 10) for q in qs]
    seeds = cr.seeds_from_smems(oi, qs, per, 0, 30)
    want = [cr.chain_query(s, [int(x) for x in st], P)[:2] for s in seeds]
    assert sum(1 for _, c in want if c) >= 400
    assert_batch_equals(ix.parallel_chains_csr(*pack_queries(qs), 10, 30, *P), want)
    ix.close()


# ---- the chunk driver's rarely taken branches, on 64 reads of 101 letters ------------------------------------------------------------

from tests.test_smems_gpu import all_equal, shrunk_cap, small_reads, with_bad_read  # noqa: E402

NO_CHAIN = E2E_PARAMS[(12, 20)]._replace(min_score=10 ** 6)  # above any reachable score


def assert_no_chains(got, n):
    off, ch, soff, sd, st = got
    assert np.array_equal(off, np.zeros(n + 1, np.uint64)) and len(ch) == 0 and np.array_equal(soff, [0]) and len(sd) == 0
    assert st.dtype == np.uint8 and np.array_equal(st, np.zeros(n, np.uint8))


def test_chunks_without_smems_and_without_chains_give_zero_offsets_and_ok_status(nt):
    reads = small_reads(nt)
    qb, qo = pack_queries(reads)
    assert_no_chains(nt.ix.parallel_chains_csr(qb, qo, 102, 20, *E2E_PARAMS[(12, 20)]), len(reads))  # min_len above every read's length
    assert int(nt.ix.parallel_locate_smems_csr(qb, qo, 20, 12)[2][-1]) >= len(reads)  # seeds, and no chain of them
    assert_no_chains(nt.ix.parallel_chains_csr(qb, qo, 12, 20, *NO_CHAIN), len(reads))


def test_a_bad_read_is_named_before_the_capacity_test_splits_its_chunk(nt):
    reads = small_reads(nt, 6)
    with shrunk_cap("AWRY_ANCHOR_HIT_CAP"):
        for bad in (b"AC$T", b"", bytes([0x41, 0x80])):
            with pytest.raises(AwryError) as e:
                nt.ix.parallel_chains_csr(*pack_queries(with_bad_read(reads, bad)), 12, 20, *E2E_PARAMS[(12, 20)])
            assert e.value.code == ERR_INVALID_QUERY and "query 3:" in str(e.value), bad


def test_seven_reads_halved_down_to_single_reads_equal_the_uncapped_call(nt):
    qb, qo = pack_queries(small_reads(nt, 7))
    want = nt.ix.parallel_chains_csr(qb, qo, 12, 20, *E2E_PARAMS[(12, 20)])
    assert int(want[0][-1]) >= 7
    with shrunk_cap("AWRY_ANCHOR_HIT_CAP"):
        assert all_equal(want, nt.ix.parallel_chains_csr(qb, qo, 12, 20, *E2E_PARAMS[(12, 20)]))


def test_every_member_seed_is_a_located_hit_of_an_smem_of_the_same_read(nt):
    reads = small_reads(nt)
    qb, qo = pack_queries(reads)
    off, ch, soff, sd, st = nt.ix.parallel_chains_csr(qb, qo, 12, 20, *E2E_PARAMS[(12, 20)])
    moff, sm, hoff, g, _ = nt.ix.parallel_locate_smems_csr(qb, qo, 20, 12)
    assert not st.any() and int(np.diff(off.astype(np.int64)).max()) >= 2  # no read abandoned, and one of at least two chains
    for i in range(len(reads)):
        hits = {(int(sm[s]["q_begin"]), int(sm[s]["q_len"]), int(t)) for s in range(int(moff[i]), int(moff[i + 1])) for t in g[int(hoff[s]):int(hoff[s + 1])]}
        members = sd[int(soff[int(off[i])]):int(soff[int(off[i + 1])])]
        assert len(members) or off[i] == off[i + 1]
        for m in members:
            assert (int(m["q_begin"]), int(m["q_len"]), int(m["t_pos"])) in hits, (i, m)
