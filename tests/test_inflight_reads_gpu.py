"""The read pipelines in flight: streams, host threads, scratch growth (run on a real MI355X via `pytest -m gpu`).

tests/test_inflight_gpu.py puts the promises of include/awry_hip.h (the block above awry_replica_device) under load for the count,
locate and mismatch families.  This module does the same for what came after it -- anchors, SMEMs, edit locate, edit align,
chaining, chain alignment, map, pairs and the clipped modes -- and keeps that module's rules: every expected array comes from the CPU
references (tests/anchor_ref.py, smem_ref.py, edit_ref.py, align_ref.py, chain_ref.py, chain_align_ref.py, clip_ref.py, map_ref.py,
pair_ref.py, pair_clip_ref.py, mismatch_ref.py and the oracle) and is computed before anything is queued; no GPU result is the
reference for another; every comparison is bit-exact, guard words included; every stream and thread carries different data; every
output buffer is pre-filled with a sentinel.  Inputs, packing helpers, device jobs and assertions are those of the module that owns
each kernel; the long first launch and the count, locate and mismatch jobs are tests/test_inflight_gpu.py's.

  1  every user of per-stream scratch, and the scratch-free entry points, on four streams, all queued before anything is waited for
  2  edit_masks, align_trace, chain_slabs and chain_align_lists grow, shrink and change owner while work is queued on their stream;
     the growth plan is worked out from the sizing rules of launchers.h before anything is queued, and asserted
  3  twelve host threads inside the batch calls (every read pipeline driver runs on the replica's one stream) beside two threads with
     streams of their own: default capacities, capacities of a few items (many launches and halvings), two replicas on one GPU
  4  the first use of the edit scan's private text copy from three threads at once, beside two streams of count jobs
  5  one stream -- a created one, then the NULL stream -- driven by two host threads; the ring of work-queue heads wraps several times

Nothing here depends on timing: the long first launch and the barriers only raise the chance of overlap, and whether the first launch
was still running when the last one was queued is printed, not asserted.

Wall times on one MI355X (256 CUs), from one sitting of the whole suite (460 passed in 499 s) and one of this module alone (10 passed
in 26 s, 11 s of it the session's start-up in the first setup, which the whole suite pays once: there the setup of test 1 takes 1.8 s);
call of the slowest case of each test:
  fixtures: world 0.4 s, material 0.8 s, 80 jobs for four streams 0.8 s, long first launch 0.2 s, the twelve batch calls 1.9 s
  1  four streams 0.56 s (first round 285 ms to queue on fresh scratch, second 2.1 ms with the first launch still running)
  2  growth 0.46 s on one stream, 0.54 s on two
  3  host threads 1.3 s at the default capacities, 4.1 s at the small ones, 1.2 s with two replicas
  4  first use of the text copy 0.25 s
  5  one stream from two threads 0.62 s (created stream), 0.60 s (NULL stream)
"""
import contextlib
import os
import threading
import time

import numpy as np
import pytest

from awry_amd.fm_index import ALIGN_MAX_OPS, ANCHOR_DTYPE, MAP_CLIP_DTYPE, MAP_DTYPE, FmIndex, pack_queries
from tests import align_ref as al
from tests import anchor_ref as ar
from tests import chain_ref as cr
from tests import clip_ref as cl
from tests import edit_ref as er
from tests import map_ref as mp
from tests import mismatch_ref
from tests import pair_clip_ref as pc
from tests import pair_ref as pr
from tests import synth
from tests import test_chain_align_gpu as cag
from tests import test_chain_gpu as cg
from tests import test_clip_gpu as clg
from tests import test_edit_gpu as eg
from tests import test_map_gpu as mg
from tests import test_pair_clip_gpu as pcg
from tests import test_pair_gpu as pg
from tests.test_anchors_gpu import nt_queries
from tests.test_grid_trips_gpu import chain_cases
from tests.test_inflight_gpu import THREADS, _interleave, _mix, _sampled_chunked, _streams, heavy_job, kmer_job, locate_ascii_job, mismatch_job
from tests.test_map_cpu import fixture_reads, hand_made_lists
from tests.test_pair_gpu import lists_ix  # noqa: F401  (a fixture: the index whose records are the hand-made pair lists')

pytestmark = pytest.mark.gpu

KEY, P_MAIN = cag.KEY, mg.P_MAIN
MAX_HITS = 500
GUARD = 1024         # bytes behind every output that must keep the sentinel
BLOCKER_READS, BLOCKER_TILES = 2_000_000, 20
ROUNDS = 3
SMALL_CAPS = dict(AWRY_ANCHOR_HIT_CAP="64", AWRY_CHAIN_ALIGN_SUB_BATCH="7", AWRY_EDIT_CANDIDATE_CAP="20", AWRY_ALIGN_SUB_BATCH="7")


# ---- device jobs ---------------------------------------------------------------------------------------------------------------------

class Dev:
    """the device buffers of one job: inputs uploaded, every output pre-filled with 0xEE and compared with what the reference
    expects, the GUARD bytes behind it included"""

    def __init__(self, ix):
        self.ix, self.ptrs, self.outs = ix, [], []

    def up(self, a):
        p = self.ix.dev_upload(np.ascontiguousarray(a))
        self.ptrs.append(p)
        return p

    def tmp(self, nbytes):
        p = self.ix.dev_malloc(nbytes)
        self.ptrs.append(p)
        return p

    def out(self, label, want, mask=None, decode=None):
        """mask: the entries the launch defines (the rest may hold anything); decode: raw bytes -> what `want` is compared with"""
        want = np.ascontiguousarray(want)
        nbytes = want.nbytes if decode is None else decode[0]
        p = self.tmp(nbytes + GUARD)
        self.ix.dev_memset(p, 0xEE, nbytes + GUARD)
        self.outs.append((label, p, want, nbytes, mask, decode[1] if decode else None))
        return p

    def check(self, where):
        for label, p, want, nbytes, mask, decode in self.outs:
            raw = self.ix.dev_download(p, (nbytes + GUARD,), np.uint8)
            assert np.all(raw[nbytes:] == 0xEE), "%s: %s: written past its end" % (where, label)
            if decode is not None:
                got = decode(raw[:nbytes])
            elif want.dtype.names:
                got = raw[:nbytes].view(want.dtype)
                for f in want.dtype.names:
                    bad = np.nonzero(got[f] != want[f])[0]
                    assert not len(bad), "%s: %s.%s differs from the reference, first at %d: %r, expected %r" % (where, label, f, bad[0], got[bad[0]], want[bad[0]])
                continue
            else:
                got = raw[:nbytes].view(want.dtype).reshape(want.shape)
            ne = got != want if mask is None else (got != want) & mask
            if ne.any():
                at = tuple(int(x[0]) for x in np.nonzero(ne))
                raise AssertionError("%s: %s differs from the reference at %d of %d entries, first at %r: %r, expected %r"
                                     % (where, label, int(ne.sum()), want.size, at, got[at], want[at]))

    def free(self):
        for p in self.ptrs:
            self.ix.dev_free(p)
        self.ptrs = []


class RJob:
    """one job of this module: build(dev, stream) uploads, allocates and returns what queues the launches"""

    def __init__(self, name, build, heads=0):
        self.name, self.build, self.heads = name, build, heads

    def prepare(self, ix, s):
        self.dev = Dev(ix)
        self.run = self.build(ix, self.dev, s)

    def queue(self):
        self.run()

    def check(self, where):
        try:
            self.dev.check("%s %s" % (where, self.name))
        finally:
            self.dev.free()


class OwnerJob:
    """a device job of the module that owns the kernel (its device_job / run_job / job_result and its assertion)"""

    def __init__(self, name, make, run, result, verify, heads=0):
        self.name, self.make, self.run, self.result, self.verify, self.heads = name, make, run, result, verify, heads

    def prepare(self, ix, s):
        self.ix, self.j = ix, self.make(ix, s)

    def queue(self):
        self.run(self.ix, self.j)

    def check(self, where):
        got = self.result(self.ix, self.j)
        try:
            self.verify(got, self.j)
        except AssertionError as e:
            raise AssertionError("%s %s: %s" % (where, self.name, e)) from e


class TorchJob:
    """a job of tests/test_inflight_gpu.py (dev_locate behind its count and scan, dev_count_mismatch, dev_count_nt2)"""

    def __init__(self, job):
        self.name, self.job, self.heads = job.name, job, job.heads

    def prepare(self, ix, s):
        self.ix, self.s = ix, s
        self.job.reset()

    def queue(self):
        self.job.queue({"nt": (self.ix, 0)}, self.s)

    def check(self, where):
        self.job.check(where)


def scan_scratch(ix, dev, n):
    return dev.tmp(ix.dev_scan_scratch_bytes(max(n, 1)))


def padded(qb):
    return np.concatenate([qb, np.zeros(16, np.uint8)])


def edit_windows_job(w, qs, wins, k):
    """dev_edit_windows in both passes on the windows [(query, first, count)]"""
    m = len(wins)
    memo = {}
    for win in wins:
        if win not in memo:
            qi, first, count = win
            memo[win] = er.hits_of(w.t.D(qs[qi]), k, first, first + count) if len(qs[qi]) > k else (np.zeros(0, np.int64), np.zeros(0, np.uint8))
    n_hits = np.array([len(memo[x][0]) for x in wins], np.uint64)
    off = np.zeros(m + 1, np.uint64)
    off[1:] = np.cumsum(n_hits)
    g = np.concatenate([memo[x][0] for x in wins]).astype(np.uint64)
    e = np.concatenate([memo[x][1] for x in wins]).astype(np.uint8)
    qb, qo = pack_queries(qs)
    cols = [np.array([x[c] for x in wins], t) for c, t in ((0, np.uint32), (1, np.uint64), (2, np.uint32))]

    def build(ix, dev, s):
        ptrs = [dev.up(a) for a in [padded(qb), qo] + cols]
        d_n, d_off, d_g, d_e = dev.out("hits per window", n_hits), dev.out("hit offsets", off), dev.out("hit positions", g), dev.out("hit distances", e)
        d_scr = scan_scratch(ix, dev, m)

        def run():
            ix.dev_edit_windows(*ptrs, m, k, d_n, None, None, None, s)
            ix.dev_scan_counts(d_n, m, d_off, d_scr, s)
            ix.dev_edit_windows(*ptrs, m, k, None, d_off, d_g, d_e, s)
        return run
    return RJob("dev_edit_windows k=%d m=%d hits=%d" % (k, m, len(g)), build)


def edit_align_job(w, qs, triples, k, memo):
    """dev_edit_align on the triples [(query, start, distance)]; memo: the reference per distinct (read, start, distance)"""
    m = len(triples)
    tl, n_ops = np.zeros(m, np.uint32), np.zeros(m, np.uint8)
    ops, defined = np.zeros((m, ALIGN_MAX_OPS), np.uint32), np.zeros((m, ALIGN_MAX_OPS), bool)
    for h, (qi, s0, d) in enumerate(triples):
        key = (qs[qi], s0, d)
        if key not in memo:
            memo[key] = al.align_triple(w.t, qs[qi], s0, d) if len(qs[qi]) > k and d <= k else (0, np.zeros(0, np.uint32))
        wtl, wruns = memo[key]
        tl[h], n_ops[h] = wtl, len(wruns)
        ops[h, :len(wruns)], defined[h, :len(wruns)] = wruns, True
    qb, qo = pack_queries(qs)
    cols = [np.array([x[c] for x in triples], t) for c, t in ((0, np.uint32), (1, np.uint64), (2, np.uint8))]

    def build(ix, dev, s):
        ptrs = [dev.up(a) for a in [padded(qb), qo] + cols]
        d_tl, d_n, d_ops = dev.out("text lengths", tl), dev.out("run counts", n_ops), dev.out("runs", ops, mask=defined)
        return lambda: ix.dev_edit_align(*ptrs, m, k, d_tl, d_n, d_ops, s)
    return RJob("dev_edit_align k=%d m=%d aligned=%d" % (k, m, int((n_ops > 0).sum())), build)


def chain_seeds_job(w, sets, order, P, memo):
    """dev_chain_seeds in both passes (tests/test_chain_gpu.py's device job) on the seed sets sets[i] for i in order"""
    st = [int(x) for x in w.st]
    for i in set(order):
        if (i, P) not in memo:
            memo[(i, P)] = cr.chain_query(sets[i], st, P)
    want = cr.as_csr([memo[(i, P)][:2] for i in order])
    tally = tuple(sum(memo[(i, P)][2][k] for i in order) for k in range(3))
    mine = [sets[i] for i in order]

    def verify(got, j):
        cg.assert_equals_reference(got, want, j["cap_c"], j["cap_m"])
        assert tuple(int(x) for x in got["t"]) == tally
    return OwnerJob("dev_chain_seeds max_seeds=%d lookback=%d n=%d" % (P.max_seeds, P.lookback, len(order)),
                    lambda ix, s: cg.device_job(ix, mine, P, s, tally=True), cg.run_job, cg.job_result, verify)


def align_chains_job(cases, ref, pick, band):
    """dev_align_chains in both passes (tests/test_chain_align_gpu.py's device job)"""
    want, packed, names = ref.many(pick, band), cag.pack_job(cases, pick), [cases[i][0] for i in pick]
    return OwnerJob("dev_align_chains band=%d m=%d" % (band, len(pick)), lambda ix, s: cag.device_job(ix, packed, band, len(want[2]), s), cag.run_job,
                    cag.job_result, lambda got, j: cag.assert_equals_reference(got, want, names))


def align_chains_clip_job(cases, ref, pick, band, wts):
    """dev_align_chains_clip in both passes (tests/test_clip_gpu.py's device job)"""
    want, packed, names = ref.many(pick, band, wts), cag.pack_job(cases, pick), [cases[i][0] for i in pick]
    return OwnerJob("dev_align_chains_clip band=%d weights=%r m=%d" % (band, wts, len(pick)),
                    lambda ix, s: clg.device_job(ix, packed, band, wts, len(want[2]), s), clg.run_job, clg.job_result,
                    lambda got, j: clg.assert_equals_reference(got, want, names))


def records_job(what, qs, per_query, min_len, skip=0):
    """dev_smems / dev_anchors in both passes: 24-byte records of the reads' SMEMs (anchors) of at least min_len letters"""
    n = len(qs)
    off, rows = ar.as_csr([[a for a in recs if a[1] >= min_len] for recs in per_query])
    tot = int(off[-1])
    assert all(len(q) for q in qs) and tot > 0
    qb, qo = pack_queries(qs)
    as_rows = (24 * tot, lambda raw: ar.got_as_rows(raw.view(ANCHOR_DTYPE)))

    def build(ix, dev, s):
        d_q, d_o = dev.up(padded(qb)), dev.up(qo)
        d_n, d_off, d_st = dev.out("records per read", np.diff(off)), dev.out("record offsets", off), dev.out("status", np.zeros(n, np.uint8))
        d_a, d_scr = dev.out("records", np.asarray(rows, np.int64).reshape(-1, 4), decode=as_rows), scan_scratch(ix, dev, n)
        if what == "smems":
            launch = lambda *a: ix.dev_smems(d_q, d_o, n, min_len, *a, s)
        else:
            launch = lambda *a: ix.dev_anchors(d_q, d_o, n, min_len, skip, *a, s)

        def run():
            launch(d_n, None, None, d_st)
            ix.dev_scan_counts(d_n, n, d_off, d_scr, s)
            launch(None, d_off, d_a, None)
        return run
    return RJob("dev_%s min_len=%d n=%d records=%d" % (what, min_len, n, tot), build)


def revcomp_job(reads, lead):
    """dev_revcomp; the offsets begin at `lead`, as a slice of a larger batch would"""
    qb, qo = pack_queries(reads)
    wb, wo = pack_queries(mp.doubled(reads))

    def build(ix, dev, s):
        d_q, d_qo = dev.up(np.concatenate([np.zeros(lead, np.uint8), padded(qb)])), dev.up(qo + np.uint64(lead))
        d_ob, d_oo = dev.out("doubled bytes", wb), dev.out("doubled offsets", wo)
        return lambda: ix.dev_revcomp(d_q, d_qo, len(reads), d_ob, d_oo, s)
    return RJob("dev_revcomp n=%d lead=%d" % (len(reads), lead), build)


def map_select_job(st, inp, want, A, R, clip=None):
    """dev_map_select (clip None) or dev_map_select_clip with clip = (match, mismatch, gap, end_bonus, min_aln_score), both passes"""
    off, alns, chains, status, n = inp
    woff, wrec, wsel, wst = want
    rec_dtype = MAP_DTYPE if clip is None else MAP_CLIP_DTYPE
    wrec = np.asarray(wrec, rec_dtype)

    def build(ix, dev, s):
        ins = (dev.up(off), dev.up(alns.view(np.uint8)), dev.up(chains.view(np.uint8)), dev.up(status))
        d_nm, d_rs, d_mo = dev.out("records per read", np.diff(woff)), dev.out("read status", np.asarray(wst, np.uint8)), dev.out("record offsets", woff)
        d_mp, d_sel = dev.out("records", wrec), dev.out("selected alignments", np.array(wsel, np.uint32))
        d_pos, d_scr = dev.out("positions", mg.positions_of(st, wrec["t_begin"])), scan_scratch(ix, dev, n)
        if clip is None:
            launch = lambda *a: ix.dev_map_select(*ins, n, A, R, *a, s)
        else:
            launch = lambda *a: ix.dev_map_select_clip(*ins, n, A, R, *clip, *a, s)

        def run():
            launch(d_nm, d_rs, None, None, None, None)
            ix.dev_scan_counts(d_nm, n, d_mo, d_scr, s)
            launch(None, None, d_mo, d_mp, d_sel, d_pos)
        return run
    return RJob("dev_map_select%s A=%d R=%d n=%d records=%d" % ("" if clip is None else "_clip", A, R, n, len(wrec)), build)


def pair_jobs(mod, P, G, seed, k):
    """dev_pair_windows and dev_pair_select in both passes on the lists of tests/test_pair_gpu.py (mod = pg) or, in the clipped mode,
    tests/test_pair_clip_gpu.py (mod = pcg): the hand-made pairs and random ones"""
    clip = mod is pcg
    hand = mod.with_slots(mod.hand_made_pairs(), G)
    pairs = hand + mod.random_pairs(P - len(hand), seed, G)
    inp = mod.pair_inputs(pairs, G)
    mn, mx, U = mod.HAND["mn"], mod.HAND["mx"], mod.HAND["U"]
    woff, wrec, wsel, wins = mod.want_select(pairs, inp, G, mn, mx, U)
    off, cands, resc, status, qoff, kept = inp
    windows_of = pc.windows_of_clip if clip else pr.windows_of
    wwin = [x for p, pair in enumerate(pairs) for x in windows_of(kept[2 * p], kept[2 * p + 1], pair[5][0], pair[5][1], mod.ST, mod.N_TEXT, mn, mx, G, k, p)]
    assert len(wwin) == 2 * P * G
    tail = (*pcg.WTS, pcg.T_MAIN) if clip else ()
    sfx = "_clip" if clip else ""

    def build_select(ix, dev, s):
        ins = (dev.up(off), dev.up(cands.view(np.uint8)), dev.up(resc.view(np.uint8)), dev.up(status))
        d_nm, d_mo, d_mp = dev.out("records per read", np.diff(woff)), dev.out("record offsets", woff), dev.out("records", wrec)
        d_sel, d_pos = dev.out("selected candidates", wsel), dev.out("positions", mg.positions_of(mod.ST, wrec["t_begin"]))
        d_ins, d_scr = dev.out("inserts", wins), scan_scratch(ix, dev, 2 * P)
        launch = getattr(ix, "dev_pair_select" + sfx)

        def run():
            launch(*ins, P, mn, mx, U, G, *tail, d_nm, None, None, None, None, None, s)
            ix.dev_scan_counts(d_nm, 2 * P, d_mo, d_scr, s)
            launch(*ins, P, mn, mx, U, G, *tail, None, d_mo, d_mp, d_sel, d_pos, d_ins, s)
        return run

    def build_windows(ix, dev, s):
        ins = (dev.up(off), dev.up(cands.view(np.uint8)), dev.up(qoff))
        outs = [dev.out(label, np.array([x[c] for x in wwin], t)) for c, (label, t) in enumerate((("window queries", np.uint32), ("window starts", np.uint64),
                                                                                                  ("window counts", np.uint32)))]
        launch = getattr(ix, "dev_pair_windows" + sfx)
        return lambda: launch(*ins, P, mn, mx, G, k, *outs, s)
    return [RJob("dev_pair_windows%s P=%d G=%d" % (sfx, P, G), build_windows), RJob("dev_pair_select%s P=%d G=%d records=%d" % (sfx, P, G, len(wrec)), build_select)]


# ---- fixtures ------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def nt(oracle):
    """the 40 000-letter world of tests/test_grid_trips_gpu.py, with what the references of every pipeline take: the symbols (tsym),
    the record starts, the edit reference's text (t) and the attributes of tests/test_edit_gpu.py's World that eg.planted reads"""
    t0 = time.time()
    w = pcg.ClipPairWorld(oracle, *synth.make_text(40_000, 0, 21, 5, 0.03), 0)
    w.starts, w.n, w.letters = [int(v) for v in w.st], w.t.n, synth.NT
    print("[inflight reads] world: %.2f s" % (time.time() - t0))
    return w


@pytest.fixture(scope="module")
def blocker(nt):
    """tests/test_inflight_gpu.py's long first launch: the generic kernel over two million 101-bp reads with row intervals (100 000
    reads from the text, twenty times over: the oracle counts each once)"""
    t0 = time.time()
    q2d = _sampled_chunked(nt.text, BLOCKER_READS // BLOCKER_TILES, 101, 77)
    want = nt.oi.parallel_count(*synth.fixed_to_csr(q2d), THREADS)[0]
    job = heavy_job(nt, np.tile(q2d, (BLOCKER_TILES, 1)), np.tile(want, BLOCKER_TILES))
    print("[inflight reads] blocker: %.2f s" % (time.time() - t0))
    return job


class Material:
    """what the jobs of every test are cut from, with the references memoised per distinct item"""


@pytest.fixture(scope="module")
def mat(nt):
    t0 = time.time()
    m = Material()
    rng = np.random.default_rng(70)
    # edit windows and edit alignment: planted reads of 33 .. 256 letters (the joins of the five records are avoided) and two cuts
    m.edit_qs = [eg.planted(nt, rng, L, ops, p=p)[0] for L, ops, p in (
        (101, [("s", 30), ("d", 70)], 5000), (200, [("i", 100)], 12_000), (64, [("s", 10)], 3000), (65, [("d", 20)], 7000),
        (256, [("s", 3), ("i", 128), ("s", 250)], 9000), (33, [("s", 5)], 21_000), (150, [("d", 9), ("i", 77)], 30_000))]
    m.edit_qs += [bytes(nt.text[100:140]), bytes(nt.text[15_000:15_256])]
    assert all(set(q) <= set(b"ACGTN") and 33 <= len(q) <= 256 for q in m.edit_qs)
    m.hits = {k: [(qi, int(s), int(d)) for qi, q in enumerate(m.edit_qs) for s, d in list(zip(*er.hits_of(nt.t.D(q), k)))[:12]] for k in (2, 5, 8)}
    assert all(len(v) >= 6 for v in m.hits.values()), {k: len(v) for k, v in m.hits.items()}
    m.align_memo, m.chain_memo = {}, {}
    # chain alignment: the hand-made chains of the owners' suites, 101-letter and 1024-letter ones among them
    m.cases = chain_cases(nt.text, nt.st)
    names = [c[0] for c in m.cases]
    m.short = [i for i, c in enumerate(m.cases) if len(c[1]) <= 101]
    m.long = [i for i, c in enumerate(m.cases) if len(c[1]) == 1024]
    assert len(m.long) >= 3 and len(m.short) >= 20 and any(len(m.cases[i][1]) == 101 for i in m.short), names
    m.ref, m.clip_ref = cag.Reference(nt.tsym, m.cases), clg.Reference(nt.tsym, nt.st, m.cases)
    m.sets = cg.synthetic_sets(nt.st)
    # SMEMs and anchors: the anchor suite's reads of up to 150 letters, the SMEMs from the oracle's counts
    m.reads = [q for q in dict.fromkeys(nt_queries(nt, (6, nt.ix.seed_kmer_len()))) if len(q) <= 150]
    m.smems = {q: nt.ref(q) for q in m.reads}
    m.anchors = {q: ar.anchors_definition(nt.ctext, nt.oi, q, 0, 1, 0) for q in m.reads}
    m.hand_lists = [(mg.strand_lists(c), capped) for _, c, capped, _ in hand_made_lists()]
    print("[inflight reads] material: %.2f s" % (time.time() - t0))
    return m


def edit_windows_for(nt, mat, i, m, k):
    """m windows for stream i: around hits, random ones, the whole text once, the text's end, beyond it, and an empty one"""
    rng = np.random.default_rng(900 + 31 * i + k)
    n, nq = nt.n, len(mat.edit_qs)
    wins = [(0, 0, n), (1 % nq, n - 3, 10), (2, n + 7, 3), (3, 100, 0)]
    for qi, s, _ in mat.hits[k]:
        wins.append((qi, max(0, s - int(rng.integers(0, 9))), int(rng.integers(1, 30))))
    while len(wins) < m:
        wins.append((int(rng.integers(0, nq)), int(rng.integers(0, n - 400)), int(rng.integers(1, 400))))
    return [wins[j] for j in rng.permutation(len(wins))[:m]]


def edit_triples_for(nt, mat, i, m, k):
    """m triples for stream i: hits within k edits, and triples that are no alignment (a start off a hit, a start at and past n)"""
    rng = np.random.default_rng(700 + 31 * i + k)
    base = mat.hits[k] + [(0, 4999, min(k, 3)), (0, 7000, k), (7, 300, 0), (0, nt.n, k), (7, nt.n + 7, 0)]
    return [base[j] for j in rng.integers(0, len(base), size=m)]


def chain_pick_for(mat, i, m, long_every=7):
    rng = np.random.default_rng(500 + i)
    return [mat.long[int(rng.integers(0, len(mat.long)))] if j % long_every == 0 else mat.short[int(rng.integers(0, len(mat.short)))] for j in range(m)]


def stream_jobs(nt, mat, i):
    """every entry point of the read pipelines for stream i: contents of its own (seeds), an order of its own (rotation + reversal)"""
    rng = np.random.default_rng(40 + i)
    qs = [mat.reads[j] for j in rng.permutation(len(mat.reads))[:60 + 7 * i]]
    n_text = len(nt.text) - 1
    sel = mat.hand_lists + mg.random_lists(300 + 11 * i - len(mat.hand_lists), 3100 + i, n_text)
    inp = mg.select_inputs(sel)
    cinp = clg.random_select_input(300 + 13 * i, 70 + i, n_text)
    A, R = (1, 3, 8, 3)[i], (1, 6, 16, 2)[i]
    order16 = [j for j in rng.permutation(len(mat.sets))] + [int(x) for x in rng.integers(0, len(mat.sets), size=20 + i)]
    jobs = [
        edit_windows_job(nt, mat.edit_qs, edit_windows_for(nt, mat, i, 300 + 9 * i, 2), 2),
        edit_windows_job(nt, mat.edit_qs, edit_windows_for(nt, mat, i, 200 + 9 * i, 5), 5),
        edit_align_job(nt, mat.edit_qs, edit_triples_for(nt, mat, i, 400 + 13 * i, 2), 2, mat.align_memo),      # half-width 2
        edit_align_job(nt, mat.edit_qs, edit_triples_for(nt, mat, i, 300 + 13 * i, 5), 5, mat.align_memo),      # 6
        edit_align_job(nt, mat.edit_qs, edit_triples_for(nt, mat, i, 200 + 13 * i, 8), 8, mat.align_memo),      # 8: 8-byte direction words
        chain_seeds_job(nt, mat.sets, order16, cr.Params(4096, 16, 120, 6, 4), mat.chain_memo),                 # 4096 > the LDS tile: slabs
        chain_seeds_job(nt, mat.sets, order16[::-1][:25], cr.Params(4096, 64, 120, 6, 4), mat.chain_memo),      # the wave-wide groups
        chain_seeds_job(nt, mat.sets, order16[3:30], cr.Params(60, 16, 120, 6, 4), mat.chain_memo),             # within the tile: no slab
        align_chains_job(mat.cases, mat.ref, chain_pick_for(mat, i, 300 + 17 * i), (4, 0, 8, 1)[i]),
        align_chains_job(mat.cases, mat.ref, chain_pick_for(mat, i + 10, 200 + 17 * i), (8, 4, 0, 4)[i]),
        align_chains_clip_job(mat.cases, mat.clip_ref, chain_pick_for(mat, i + 20, 250 + 17 * i), (4, 8, 0, 4)[i], clg.WEIGHTS[i]),
        records_job("smems", qs, [mat.smems[q] for q in qs], (1, 12)[i % 2]),
        records_job("anchors", qs[::-1], [mat.anchors[q] for q in qs[::-1]], (12, 1)[i % 2]),
        revcomp_job(mg.revcomp_reads(257 + 9 * i, 60 + i), (0, 13)[i % 2]),
        map_select_job(nt.st, inp, mp.rank_alignments(inp[0], inp[2], inp[1], inp[3], inp[4], A, R), A, R),
        map_select_job(nt.st, cinp + (300 + 13 * i,), cl.rank_alignments(cinp[0], cinp[2], cinp[1], cinp[3], 300 + 13 * i, A, R, clg.MAIN, 30), A, R,
                       (*clg.MAIN, 30)),
    ]
    ljobs = pair_jobs(pg, 257 + 5 * i, (2, 1, 4, 2)[i], 300 + i, 4) + pair_jobs(pcg, 257 + 3 * i, (2, 4, 1, 2)[i], 700 + i, 4)
    both = [("nt", j) for j in jobs] + [("lists", j) for j in ljobs]
    k = (5 * i + 3) % len(both)
    both = both[k:] + both[:k]
    return both[::-1] if i % 2 else both


@pytest.fixture(scope="module")
def jobsets(nt, mat, lists_ix):
    t0 = time.time()
    sets = [stream_jobs(nt, mat, i) for i in range(4)]
    print("[inflight reads] %d jobs for 4 streams and their references: %.2f s" % (sum(len(x) for x in sets), time.time() - t0))
    return sets


def run_queued(idx, streams, lists, blocker=None, what=""):
    """lists[si]: the (index name, job) pairs of stream si.  Everything is prepared, the device is idle, then everything is queued --
    behind `blocker` on streams[0] -- without a wait in between; one synchronise; every output compared.  Whether the blocker was still
    running when the last launch was queued is printed (nothing depends on it)."""
    import torch
    plan = _interleave(lists)
    for si, (which, job) in plan:
        job.prepare(idx[which], streams[si].cuda_stream)
    ev = None
    if blocker is not None:
        blocker.reset()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if blocker is not None:
        blocker.queue({"nt": (idx["nt"], 0)}, streams[0].cuda_stream)
        ev = torch.cuda.Event()
        ev.record(streams[0])
    for si, (which, job) in plan:
        job.queue()
    pending = ev is not None and not ev.query()
    dt = time.perf_counter() - t0
    torch.cuda.synchronize()
    print("[inflight reads] %s: %d jobs on %d stream(s) queued in %.2f ms; the first launch was %s when the last was queued"
          % (what, len(plan), len(streams), dt * 1e3, "still running" if pending else "not running (or absent)"))
    if blocker is not None:
        blocker.check(what)
    for si, (which, job) in plan:
        job.check("%s, stream %d," % (what, si))


# ---- test 1 --------------------------------------------------------------------------------------------------------------------------

def test_every_entry_point_on_four_streams_queued_before_anything_finishes(nt, lists_ix, jobsets, blocker):
    """dev_edit_windows (edit_masks), dev_edit_align at half-widths 2, 6 and 8 (align_trace at 4 and 8 bytes a row), dev_chain_seeds with
    max_seeds above the LDS tile at both group widths (chain_slabs) and within it, dev_align_chains and dev_align_chains_clip in both
    passes (chain_align_lists, align_trace), and the scratch-free dev_smems, dev_anchors, dev_revcomp, dev_map_select[_clip],
    dev_pair_windows[_clip], dev_pair_select[_clip] -- on each of four streams, each with data, parameters and an order of its own, all
    queued behind a long first launch before anything is waited for.  The first round meets fresh scratch (every workspace is
    allocated and grown with work queued), the second the steady state."""
    idx = {"nt": nt.ix, "lists": lists_ix}
    streams = _streams(4)
    for rnd in range(2):
        run_queued(idx, streams, jobsets, blocker, "four streams, round %d" % rnd)


# ---- test 2 --------------------------------------------------------------------------------------------------------------------------

# The sizing rules of launchers.h for the device entry points, as functions of the grid the launcher picks.
def grid_for(cus, items, per_block, blocks_per_cu=8):
    return max(1, min((items + per_block - 1) // per_block, cus * blocks_per_cu))


def edit_align_trace_words(cus, m, k):
    """launch_edit_align at max_rows = 256: one direction word (4 bytes up to half-width 6, 8 at 8) per row and grid lane"""
    wb = 4 if k <= 6 else 8
    blocks = max(1, min(grid_for(cus, m, 256), (128 << 20) // (256 * wb * 256)))
    return (blocks * 256 * 256 * wb + 7) // 8


def chain_align_trace_words(cus, m):
    """launch_chain_align at max_rows = 1024: the largest of the three classes' tables (4, 8, 16 bytes a row)"""
    most = 0
    for rb in (4, 8, 16):
        blocks = max(1, min(grid_for(cus, m, 256), (512 << 20) // (1024 * rb * 256)))
        most = max(most, blocks * 256 * 1024 * rb)
    return (most + 7) // 8


def chain_align_lists_need(m):
    return 3 * m + 3


def chain_slab_bytes(cus, n, max_seeds, group=16):
    tile = 64 if group == 16 else 256
    if max_seeds <= tile:
        return 0
    cap = 1
    while cap < max_seeds:
        cap <<= 1
    slab = cap * 36 * (256 // group)
    return max(1, min(grid_for(cus, n, 256 // group, 4), (128 << 20) // slab)) * slab


def edit_masks_words(m):
    return m * 5 * 4  # the device entry point: masks per window, five symbols, four words


# (step kind, size, parameter): what one stream is given, in this order, without a wait in between
GROWTH_STEPS = (("edit_align", 100, 2), ("align_chains", 100, 4), ("edit_align", 3000, 8), ("edit_windows", 200, 2), ("align_chains_clip", 3000, 4),
                ("chain_seeds", 20, 100), ("edit_align", 63, 5), ("align_chains", 63, 0), ("edit_windows", 2000, 5), ("edit_align", 3001, 8),
                ("chain_seeds", 40, 4096), ("align_chains_clip", 3900, 8), ("edit_windows", 100, 2), ("edit_align", 300, 2))


def growth_plan(cus, steps=GROWTH_STEPS):
    """-> per buffer, the steps at which the launcher has to grow it on a fresh stream: [(step, need, what the stream held before)].
    The launchers keep what they have when it suffices and allocate a quarter more than they need for edit_masks and
    chain_align_lists, exactly what they need for align_trace and chain_slabs."""
    have = dict(align_trace=0, chain_align_lists=0, chain_slabs=0, edit_masks=0)
    grown = {b: [] for b in have}

    def need(buf, step, n, spare):
        if have[buf] < n:
            grown[buf].append((step, n, have[buf]))
            have[buf] = n + (n // 4 if spare else 0)
    for step, (kind, size, par) in enumerate(steps):
        if kind == "edit_align":
            need("align_trace", step, edit_align_trace_words(cus, size, par), False)
        elif kind in ("align_chains", "align_chains_clip"):
            need("chain_align_lists", step, chain_align_lists_need(size), True)
            need("align_trace", step, chain_align_trace_words(cus, size), False)
        elif kind == "chain_seeds":
            need("chain_slabs", step, chain_slab_bytes(cus, size, par), False)
        else:
            need("edit_masks", step, edit_masks_words(size), True)
    return grown


def assert_growth_plan(cus):
    """what the sequence is for, on a device of `cus` CUs: align_trace changes owner at every alignment step and grows under either
    owner -- an edit alignment's need above a queued chain alignment's, and the other way round --, it and chain_align_lists grow at
    least twice after their first allocation with smaller needs in between, and the slabs and the masks grow once more each"""
    g = growth_plan(cus)
    kinds = [s[0] for s in GROWTH_STEPS]
    users = [k for k in kinds if k != "edit_windows" and k != "chain_seeds"]
    assert all((a == "edit_align") != (b == "edit_align") for a, b in zip(users, users[1:])), users
    trace = [s for s, _, _ in g["align_trace"]]
    assert len(trace) >= 3 and any(kinds[s] == "edit_align" for s in trace[1:]) and any(kinds[s] != "edit_align" for s in trace[1:]), (cus, g["align_trace"])
    assert len(g["chain_align_lists"]) >= 3 and len(g["chain_slabs"]) >= 2 and len(g["edit_masks"]) >= 2, (cus, g)
    for buf, of in (("align_trace", ("edit_align", "align_chains", "align_chains_clip")), ("chain_align_lists", ("align_chains", "align_chains_clip"))):
        steps = [s for s, _, _ in g[buf]]  # between two growths lies a step of a user of the buffer that needs less
        assert any(kinds[s] in of for a, b in zip(steps, steps[1:]) for s in range(a + 1, b)), (cus, buf, g[buf])
    return g


def growth_jobs(nt, mat, i):
    """the steps of GROWTH_STEPS for stream i, each with data of its own"""
    jobs = []
    for step, (kind, size, par) in enumerate(GROWTH_STEPS):
        sd = 100 * i + step
        if kind == "edit_align":
            jobs.append(edit_align_job(nt, mat.edit_qs, edit_triples_for(nt, mat, sd, size, par), par, mat.align_memo))
        elif kind == "align_chains":
            jobs.append(align_chains_job(mat.cases, mat.ref, chain_pick_for(mat, sd, size, 2 if size > 1000 else 50), par))  # 1024-letter queries
        elif kind == "align_chains_clip":
            jobs.append(align_chains_clip_job(mat.cases, mat.clip_ref, chain_pick_for(mat, sd, size, 50 if size > 3500 else 3), par, clg.MAIN))
        elif kind == "chain_seeds":
            rng = np.random.default_rng(sd)
            order = [int(x) for x in rng.integers(0, len(mat.sets), size=size)]
            jobs.append(chain_seeds_job(nt, mat.sets, order, cr.Params(par, 16, 120, 6, 4), mat.chain_memo))
        else:
            jobs.append(edit_windows_job(nt, mat.edit_qs, edit_windows_for(nt, mat, sd, size, par), par))
    return [("nt", j) for j in jobs]


def test_the_growth_plan_holds_at_256_cus():
    g = assert_growth_plan(256)
    assert len(g["align_trace"]) - 1 >= 2 and len(g["chain_align_lists"]) - 1 >= 2


@pytest.mark.parametrize("nstreams", [1, 2])
def test_workspaces_grow_and_change_owner_while_work_is_queued(nt, mat, blocker, nstreams):
    """GROWTH_STEPS on one fresh stream without a wait from the test, then two such sequences interleaved over two fresh streams.
    align_trace changes owner and word width at every alignment step; it, chain_align_lists, chain_slabs and edit_masks grow where
    the plan says (asserted for this device's CU count before anything is queued), with alignments of the other kind, chainings and
    scans queued in front of the growth and behind it.  (The streams are fresh for this replica: the module creates 17 streams in all,
    fewer than the 32 of torch's pool, so none comes back.)"""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    g = assert_growth_plan(cus)
    print("[inflight reads] growth plan at %d CUs: %r" % (cus, g))
    lists = [growth_jobs(nt, mat, 10 * nstreams + i) for i in range(nstreams)]
    run_queued({"nt": nt.ix}, _streams(nstreams), lists, blocker, "growth, %d stream(s)" % nstreams)


# ---- test 3 --------------------------------------------------------------------------------------------------------------------------

def want_alignments_clip(nt, qs, chains_per, max_alignments, W, wts, memo):
    """tests/test_chain_align_gpu.py's want_alignments in the clipped mode: what awry_align_chains_clip_batch returns"""
    off, rows, alns, coff, runs, st = [0], [], [], [0], [np.zeros(0, np.uint32)], []
    for q, (status, chains) in zip(qs, chains_per):
        st.append(status)
        take = chains[:max_alignments]
        for c in take:
            key = (bytes(q), tuple(c[6]), W, wts)
            if key not in memo:
                memo[key] = cl.align_chain(nt.tsym, nt.starts, cag.symbols(q), list(c[6]), W, wts)
            s, tb, te, ed, r, _, score, c_l, c_r = memo[key]
            rows.append(c[:6])
            alns.append((tb, te, ed, s, score, c_l, c_r))
            runs.append(cl.encode(r))
            coff.append(coff[-1] + len(r))
        off.append(off[-1] + len(take))
    return (np.array(off, np.uint64), np.array(rows, np.int64).reshape(-1, 6), np.array(alns, cl.ALN_CLIP_NP), np.array(coff, np.uint64), np.concatenate(runs),
            np.array(st, np.uint8))


def same(name, got, want):
    assert len(got) == len(want), name
    for j, (a, b) in enumerate(zip(got, want)):
        assert np.array_equal(a, b), "%s: array %d differs from the reference" % (name, j)


@pytest.fixture(scope="module")
def batch_calls(nt, mat):
    """the twelve batch calls, each with reads of its own and its reference: name -> call(ix), which raises where the answer differs"""
    t0 = time.time()
    calls = {}
    fixture = [r[0] for r in fixture_reads(nt.text)]
    take = lambda pool, i, n: [pool[(37 * i + 3 * j) % len(pool)] for j in range(n)]
    memo, amemo, cmemo, clmemo, pmemo, pcmemo = {}, {}, {}, {}, {}, {}
    chains = nt.chains_of(P_MAIN)

    def anchors_like(name, per_query, qs, call):
        qb, qo = pack_queries(qs)
        full = [per_query[q] for q in qs]
        woff, wrows = ar.as_csr(full)
        whoff, wg, wp = ar.locate_reference(nt.oi, qs, full, 0, MAX_HITS)

        def run(ix):
            off, rec, hoff, g, p = call(ix, qb, qo)
            same(name, (off, ar.got_as_rows(rec), hoff, g, p), (woff, np.asarray(wrows, np.int64).reshape(-1, 4), whoff, wg, wp))
        calls[name] = run
    anchors_like("parallel_locate_anchors_csr", mat.anchors, take(mat.reads, 1, 80), lambda ix, qb, qo: ix.parallel_locate_anchors_csr(qb, qo, MAX_HITS, 1, 0))
    anchors_like("parallel_locate_smems_csr", mat.smems, take(mat.reads, 2, 80), lambda ix, qb, qo: ix.parallel_locate_smems_csr(qb, qo, MAX_HITS, 1))

    qs3 = take(fixture, 3, 64) + take(mat.reads, 3, 30)
    per3 = chains(qs3)
    calls["parallel_chains_csr"] = lambda ix: cg.assert_batch_equals(ix.parallel_chains_csr(*pack_queries(qs3), *KEY, *P_MAIN), per3)

    def edit_pool(seed):
        rng = np.random.default_rng(seed)
        qs = []
        for L in (20, 63, 64, 65, 101, 128, 129, 192, 193, 256):
            qs += eg.reads_for(nt, rng, L, 2)[0][:3]
        return [q for q in qs if set(q) <= set(b"ACGTN")]
    for name, seed, aligned in (("parallel_locate_edit_csr", 7, False), ("parallel_align_edit_csr", 8, True)):
        qs = edit_pool(seed)
        off, g, d, st, tl, coff, runs = al.align(nt.t, qs, 2, eg.NO_CAP)
        assert not st.any() and len(g) >= len(qs)
        pos = mg.positions_of(nt.st, g)

        def run(ix, name=name, qs=qs, want=(off, g, pos, d, st, tl, coff, runs), aligned=aligned):
            if aligned:
                same(name, ix.parallel_align_edit_csr(*pack_queries(qs), 2, eg.NO_CAP), want)
            else:
                same(name, ix.parallel_locate_edit_csr(*pack_queries(qs), 2, eg.NO_CAP), want[:5])
        calls[name] = run

    qs6 = take(fixture, 6, 64) + [q for q in take(mat.reads, 6, 20)]
    want6 = cag.want_alignments(nt.tsym, qs6, chains(qs6), 3, 4, amemo)
    calls["parallel_align_chains_csr"] = lambda ix: cag.assert_batch_equals(ix.parallel_align_chains_csr(*pack_queries(qs6), *KEY, 3, 4, *P_MAIN), want6)

    qs7 = take(fixture, 7, 64) + [q for q in take(mat.reads, 7, 20)]
    want7 = want_alignments_clip(nt, qs7, chains(qs7), 3, 4, clg.MAIN, cmemo)

    def align_chains_clip(ix):
        off, ch, aln, coff, cgr, st = ix.parallel_align_chains_clip_csr(*pack_queries(qs7), *KEY, 3, 4, *clg.MAIN, *P_MAIN)
        woff, wrows, waln, wcoff, wruns, wst = want7
        same("parallel_align_chains_clip_csr", (off, st, cr.got_chain_rows(ch), coff, cgr) + tuple(aln[f] for f in cl.ALN_CLIP_NP.names),
             (woff, wst, wrows, wcoff, wruns) + tuple(waln[f] for f in cl.ALN_CLIP_NP.names))
    calls["parallel_align_chains_clip_csr"] = align_chains_clip

    r8 = take(fixture, 8, 64)
    want8 = mg.want_maps(nt, r8, 3, 6, 4, P_MAIN, memo)
    calls["parallel_map_csr"] = lambda ix: mg.assert_maps_equal(ix.parallel_map_csr(*pack_queries(r8), *KEY, 3, 6, 4, *P_MAIN), want8, nt.st, "map")
    r9 = take(fixture, 9, 64)
    want9 = clg.want_maps(nt, r9, 3, 6, 4, clg.MAIN, 0, clmemo)
    calls["parallel_map_clip_csr"] = lambda ix: clg.assert_maps_equal(clg.got_maps(ix, r9, 3, 6, 4, clg.MAIN, 0), want9, nt.st, "map, clipped")

    p10 = pg.interleaved(pg.fixture_pairs(nt.text, nt.st)[40:72])
    want10 = nt.want(p10, 3, 4, P_MAIN, pg.PAIR_ARGS, pmemo)[0]
    calls["parallel_map_pairs_csr"] = lambda ix: pg.assert_pairs_equal(nt.got(p10, 3, 4, P_MAIN, pg.PAIR_ARGS, ix=ix), want10, nt.st, "pairs")
    p11 = pcg.interleaved(pcg.fixture_pairs(nt.text, nt.st)[100:132])
    want11 = nt.want_clip(p11, 3, 4, P_MAIN, pcg.PAIR_ARGS, pcg.WTS, pcg.T_MAIN, pcmemo)[0]
    calls["parallel_map_pairs_clip_csr"] = lambda ix: pcg.assert_pairs_equal(nt.got_clip(p11, 3, 4, P_MAIN, pcg.PAIR_ARGS, pcg.WTS, pcg.T_MAIN, ix=ix), want11,
                                                                             nt.st, "pairs, clipped")

    mq = _mix(nt.text, 120, 18, 8101)
    mqb, mqo = synth.fixed_to_csr(mq)
    _, _, m_off, m_g, m_p, m_d = mismatch_ref.oracle_search_batch(nt.oi, [bytes(q) for q in mq], 1, 0, THREADS, True)
    calls["parallel_locate_mismatch_csr"] = lambda ix: same("parallel_locate_mismatch_csr", ix.parallel_locate_mismatch_csr(mqb, mqo, 1), (m_off, m_g, m_p, m_d))
    assert len(calls) == 12
    print("[inflight reads] twelve batch calls and their references: %.2f s" % (time.time() - t0))
    return calls


class Guard:
    """exceptions per thread, as tests/test_inflight_gpu.py's test_host_threads_mixed_with_streams collects them"""

    def __init__(self, barrier=None):
        self.errors, self.lock, self.barrier = [], threading.Lock(), barrier  # (a thread that fails releases those that wait for it)

    def thread(self, fn, *a):
        def run():
            try:
                fn(*a)
            except BaseException as e:  # noqa: BLE001
                import traceback
                with self.lock:
                    self.errors.append((getattr(fn, "__name__", "call"), a[:1], repr(e), traceback.format_exc()))
                if self.barrier is not None:
                    self.barrier.abort()
        return threading.Thread(target=run)

    def join(self, threads):
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        assert not self.errors, "\n".join("%s%s: %s\n%s" % e for e in self.errors)


def device_rounds(idx, stream, jobs, rounds, who, sync=None):
    """a host thread with a stream: prepare, queue everything, wait for the stream, compare -- `rounds` times"""
    import torch
    torch.cuda.set_device(0)
    handle = None if stream is None else stream.cuda_stream
    for rnd in range(rounds):
        for which, job in jobs:
            job.prepare(idx[which], handle)
        idx["nt"].dev_synchronize()  # (the pre-fills ran on the NULL stream)
        if sync is not None:
            sync.wait()
        for _, job in jobs:
            job.queue()
        if stream is None:
            idx["nt"].dev_synchronize()
        else:
            stream.synchronize()
        for _, job in jobs:
            job.check("%s, round %d," % (who, rnd))


@contextlib.contextmanager
def environment(values):
    old = {k: os.environ.get(k) for k in values}
    os.environ.update(values)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.mark.parametrize("mode", ["default_capacities", "small_capacities", "two_replicas"])
def test_host_threads_inside_the_batch_calls(nt, lists_ix, jobsets, batch_calls, mode):
    """Twelve threads, one per batch call, three rounds each against one index: every driver queues its launches, copies and waits on
    the replica's one stream and shares that stream's scratch and head ring with the other eleven.  Two more threads run the device
    entry points of test 1 on streams of their own.  With capacities of 64 hits, 20 candidates and sub-batches of 7 every call makes
    many launches, halvings and waits, and the head ring wraps across threads; with two replicas on one GPU the batch calls shard."""
    ix = nt.ix
    if mode == "two_replicas":
        ix = FmIndex.from_text(nt.text, 0, 8, 0, nt.st, nt.hd).set_devices([0, 0])
        assert ix.num_devices() == 2
    try:
        idx = {"nt": ix, "lists": lists_ix}
        streams = _streams(2)
        guard = Guard()

        def batch_thread(name):
            for rnd in range(ROUNDS):
                batch_calls[name](ix)
        threads = [guard.thread(batch_thread, name) for name in batch_calls]
        threads += [guard.thread(device_rounds, idx, streams[i], jobsets[i], ROUNDS, "device thread %d" % i) for i in range(2)]
        assert len(threads) == 14
        with environment(SMALL_CAPS if mode == "small_capacities" else {}):  # set before the threads start, restored after the join
            guard.join(threads)
    finally:
        if ix is not nt.ix:
            ix.close()


# ---- test 4 --------------------------------------------------------------------------------------------------------------------------

def test_first_use_of_the_private_text_copy_under_load(nt, mat, batch_calls):
    """A fresh index without the verify accelerators keeps no text8: the first call that reaches the edit scan builds the replica's
    private copy on the replica's stream.  Here that first call comes from three threads at once, released by one barrier --
    parallel_locate_edit_csr, parallel_map_pairs_csr (its rescue scans) and dev_edit_windows on a caller's stream -- while two more
    streams run k-mer counts.  A second round follows on the built copy."""
    ix = FmIndex.from_text(nt.text, 0, 8, 0, nt.st, nt.hd).set_devices([0])
    try:
        ix.set_verify(-1)  # before any thread starts: the knobs are not safe beside running queries
        assert not ix.verify_enabled()
        idx = {"nt": ix}
        streams = _streams(3)
        windows = [[("nt", edit_windows_job(nt, mat.edit_qs, edit_windows_for(nt, mat, 50 + r, 300, 2), 2))] for r in range(2)]
        counts = [[[("nt", TorchJob(kmer_job(nt, 20_000 + 999 * j + r, (31, 24)[j], 6000 + 10 * j + r, None)))] for j in range(2)] for r in range(2)]
        for rnd in range(2):
            barrier = threading.Barrier(5)
            guard = Guard(barrier)

            def batch(name):
                barrier.wait()
                batch_calls[name](ix)
            threads = [guard.thread(batch, "parallel_locate_edit_csr"), guard.thread(batch, "parallel_map_pairs_csr"),
                       guard.thread(device_rounds, idx, streams[0], windows[rnd], 1, "edit windows, round %d" % rnd, barrier)]
            threads += [guard.thread(device_rounds, idx, streams[1 + j], counts[rnd][j], 1, "counts %d, round %d" % (j, rnd), barrier) for j in range(2)]
            guard.join(threads)
    finally:
        ix.close()


# ---- test 5 --------------------------------------------------------------------------------------------------------------------------

def one_stream_jobs(nt, mat, t):
    """what thread t queues per round: dev_locate (behind its count and scan) and dev_count_mismatch ten times each -- a work-queue
    head per launch --, dev_edit_align, dev_align_chains and dev_chain_seeds twice each"""
    jobs = []
    for j in range(10):
        jobs.append(TorchJob(locate_ascii_job(nt, 300 + 10 * t + j, 2000 + 100 * t + j)))
        jobs.append(TorchJob(mismatch_job(nt, 60 + 5 * t + j, 16, 1 + j % 2, 2500 + 100 * t + j)))
        if j % 5 == 1:
            jobs.append(edit_align_job(nt, mat.edit_qs, edit_triples_for(nt, mat, 60 + 10 * t + j, 300 + j, (2, 8)[t]), (2, 8)[t], mat.align_memo))
            jobs.append(align_chains_job(mat.cases, mat.ref, chain_pick_for(mat, 60 + 10 * t + j, 280 + j), (4, 0)[t]))
            order = [int(x) for x in np.random.default_rng(60 + 10 * t + j).integers(0, len(mat.sets), size=24 + j)]
            jobs.append(chain_seeds_job(nt, mat.sets, order, cr.Params(4096, 16, 120, 6, 4), mat.chain_memo))
    assert sum(j.heads for j in jobs) >= 20  # the ring of eight heads wraps at least twice per thread and round
    return [("nt", j) for j in jobs]


@pytest.mark.parametrize("which", ["created_stream", "null_stream"])
def test_one_stream_from_two_host_threads(nt, mat, which):
    """Two threads queue device entry points with buffers of their own on the same stream -- a created one, then the NULL stream --
    each a few dozen launches per round, twenty of them with a work-queue head; each waits for the stream and compares its own
    outputs.  The launches of the two threads interleave in whatever order the threads arrive."""
    lists = [one_stream_jobs(nt, mat, t) for t in range(2)]
    stream = _streams(1)[0] if which == "created_stream" else None
    barrier = threading.Barrier(2)
    guard = Guard(barrier)
    guard.join([guard.thread(device_rounds, {"nt": nt.ix}, stream, lists[t], ROUNDS, "%s, thread %d" % (which, t), barrier) for t in range(2)])
