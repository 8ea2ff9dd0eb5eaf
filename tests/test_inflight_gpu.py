"""Launches in flight across streams and host threads (run on a real MI355X via `pytest -m gpu`).

include/awry_hip.h promises that scratch (survivor lists, the LF list, packed words of the uniform entry point, the ring of
work-queue heads) is kept per stream, "so any number of launches may be in flight across streams", and that query entry
points may be called from several host threads at once.  Here those promises are put under load: many launches of every
scratch user are queued on several streams before anything has finished, scratch grows while work is queued, the head ring
wraps, host threads mix with streams, two replicas share one GPU.

Every expected array comes from the CPU oracle (or from tests/mismatch_ref.py, which is pinned to brute force on the CPU)
and is computed before anything is queued; no GPU result serves as the reference for another.  All comparisons are
bit-exact.  Every stream carries different data and every output buffer is pre-filled with a sentinel, so a list shared
between two streams, a list sized from the wrong launch, a head reused too early or a buffer that grew under a queued launch
changes an answer.

This module covers the count, locate and mismatch families.  tests/test_inflight_reads_gpu.py does the same, under the same rules
and behind this module's long first launch, for the read pipelines -- anchors, SMEMs, edit locate and align, chaining, chain
alignment, map, pairs and the clipped modes: every device entry point on four streams, the workspaces edit_masks, align_trace,
chain_slabs and chain_align_lists growing and changing owner with work queued, twelve host threads inside the batch calls, the
first use of the edit scan's private text copy under load, and one stream driven by two host threads."""
import os
import subprocess
import sys
import threading
import time

import numpy as np
import pytest

from awry_amd.fm_index import FmIndex
from tests import mismatch_ref, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT = 0x5A5A5A5A5A5A5A5A  # what every output word holds before its launch
NT_TEXT, AA_TEXT, AA_RECORDS = 3_000_000, 2_000_000, 300
RUNG_L = 9               # below every seed k used here (13 by policy for this text, 11 on the two-replica index)
HEAVY_N, HEAVY_L = 3_000_001, 101
GROWTH_SIZES = (5_000, 2_000_003, 63, 3_000_001)  # list_slots_per_block changes every time
THREADS = 16


def _lib():
    import awry_amd
    return awry_amd.load_library()


def _dev():
    import torch
    return torch.device("cuda", 0)


def _up(a):
    """numpy array -> device tensor (uint64 travels as int64)"""
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    return torch.from_numpy(a).to(_dev())


def _up_bytes(b):
    """query bytes with the 16 bytes of slack the kernels may read past the last query"""
    return _up(np.concatenate([np.ascontiguousarray(b, dtype=np.uint8).reshape(-1), np.zeros(16, np.uint8)]))


def _out(n, dtype="i8"):
    import torch
    return torch.empty(max(int(n), 1), dtype=torch.int64 if dtype == "i8" else torch.uint8, device=_dev())


def _mix(text, n, L, seed, alphabet=0):
    """n queries of L letters: two thirds drawn from the text, one third random, shuffled"""
    a = synth.sampled_queries(text, n - n // 3, L, seed, True, alphabet)
    b = synth.random_queries(n // 3, L, alphabet, seed + 7919)
    q = np.concatenate([a, b])
    return q[np.random.default_rng(seed).permutation(n)]


def _sampled_chunked(text, n, L, seed):
    """synth.sampled_queries for millions of reads without its all-at-once window array"""
    parts, step = [], 500_000
    for i, a in enumerate(range(0, n, step)):
        parts.append(synth.sampled_queries(text, min(step, n - a), L, seed + i, False))
    q = np.concatenate(parts)
    q[q == ord("$")] = ord("A")
    return q


def _pack_words(q2d):
    """ACGT k-mers uint8[n, L <= 32] -> uint64[n], letter j in bits [2j, 2j + 2)"""
    code = np.searchsorted(synth.NT, q2d).astype(np.uint64)
    w = np.zeros(len(q2d), np.uint64)
    for j in range(q2d.shape[1]):
        w |= code[:, j] << np.uint64(2 * j)
    return w


def _dirty(q2d, seed):
    """about one query in a hundred gets an N, a lower-case run, a 'u' or an IUPAC letter"""
    rng = np.random.default_rng(seed)
    q = q2d.copy()
    n, L = q.shape
    rows = rng.choice(n, max(4, n // 100), replace=False)
    for i, r in enumerate(rows):
        kind = i % 4
        c = int(rng.integers(0, L))
        if kind == 0:
            q[r, c] = ord("N")
        elif kind == 1:
            q[r] = np.frombuffer(bytes(q[r]).lower(), np.uint8)
        elif kind == 2:
            q[r, c] = ord("u")
        else:
            q[r, c] = ord("RYKM"[int(rng.integers(0, 4))])
    return q


def _ragged(text, n, lo, hi, seed, alphabet=0):
    """n queries of lo..hi - 1 letters cut from the text, 30 % of them overwritten with random letters -> CSR.  A query cut
    from a run of N / X would match the whole run (10^5 hits each): those are overwritten too."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(lo, hi, size=n)
    qo = np.zeros(n + 1, np.uint64)
    qo[1:] = np.cumsum(lens)
    starts = rng.integers(0, len(text) - hi - 4, size=n)
    idx = np.repeat(starts, lens) + (np.arange(int(qo[-1])) - np.repeat(qo[:-1].astype(np.int64), lens))
    qb = text[idx].copy()
    letters = synth.NT if alphabet == 0 else synth.AA
    amb = np.add.reduceat((qb == (ord("N") if alphabet == 0 else ord("X"))).astype(np.int64), qo[:-1].astype(np.int64)) > 0
    rmask = np.repeat((rng.random(n) < 0.3) | amb, lens)
    qb[rmask] = letters[rng.integers(0, len(letters), size=int(rmask.sum()))]
    qb[qb == ord("$")] = letters[0]
    return qb, qo


class Job:
    """one shape on one stream: device inputs, sentinel-filled outputs, the calls that queue it and what the oracle expects"""

    def __init__(self, name, which, queue, outputs, zeroed=(), calls=1, heads=0, keep=()):
        self.name, self.which, self._queue, self.outputs, self.zeroed = name, which, queue, outputs, zeroed
        self.calls, self.heads, self.keep = calls, heads, keep  # entry-point calls, work-queue heads taken, tensors kept alive

    def reset(self):
        for _, t, _ in self.outputs:
            t.fill_(SENT if t.element_size() == 8 else 0x5A)
        for t in self.zeroed:
            t.zero_()

    def queue(self, idx, stream, si=0):
        """idx: {"nt" / "aa": (index, replica slot)}, or a function of (which, stream number) that returns such a pair"""
        ix, slot = idx(self.which, si) if callable(idx) else idx[self.which]
        self._queue(ix, slot, stream)

    def check(self, where=""):
        for label, t, want in self.outputs:
            got = t[:want.size].cpu().numpy()
            got = got.view(np.uint64) if got.dtype == np.int64 else got
            w = np.ascontiguousarray(want).reshape(-1)
            if not np.array_equal(got, w):
                bad = np.flatnonzero(got != w)
                raise AssertionError("%s %s: %s differs from the oracle at %d of %d entries, first at %d: got %#x, expected %#x"
                                     % (where, self.name, label, len(bad), len(w), bad[0], int(got[bad[0]]), int(w[bad[0]])))


# ------------------------------------------------------------------------------------------------------------------ shapes

def kmer_job(nt, n, L, seed, mode, use_seed=True):
    """dev_count_nt2 in the policy mode (mode None) or under awry_debug_set_count_kernel(mode)"""
    q2d = _mix(nt.text, n, L, seed)
    want = nt.oi.parallel_count(*synth.fixed_to_csr(q2d), THREADS)[0]
    d_w, d_c = _up(_pack_words(q2d)), _out(n)

    def queue(ix, slot, s):
        if mode is not None:
            _lib().awry_debug_set_count_kernel(mode)
        try:
            ix.dev_count_nt2(d_w.data_ptr(), n, L, d_c.data_ptr(), use_seed, s, slot)
        finally:
            if mode is not None:
                _lib().awry_debug_set_count_kernel(-1)
    return Job("dev_count_nt2 L=%d mode=%s n=%d" % (L, mode, n), "nt", queue, [("counts", d_c, want)], heads=1 if mode == 1 else 0)


def reads_job(nt, n, L, seed):
    """dev_pack_nt2 -> dev_count_nt2_long with range starts -> dev_scan_counts -> dev_locate (range stride 1)"""
    q2d = synth.sampled_queries(nt.text, n, L, seed)
    q2d[::3] = synth.random_queries(len(q2d[::3]), L, 0, seed + 1)
    off, g, p, _ = nt.oi.parallel_locate(*synth.fixed_to_csr(q2d), THREADS)
    total, W = int(off[-1]), (L + 31) // 32
    d_a, d_w, d_bad = _up_bytes(q2d), _out(n * W), _out(1)
    d_c, d_rs, d_ho, d_g, d_p = _out(n), _out(n), _out(n + 1), _out(total), _out(2 * total)
    d_scr = _out(nt.ix.dev_scan_scratch_bytes(n) // 8 + 8)

    def queue(ix, slot, s):
        ix.dev_pack_nt2(d_a.data_ptr(), n, L, d_w.data_ptr(), d_bad.data_ptr(), s, slot)
        ix.dev_count_nt2_long(d_w.data_ptr(), n, L, d_c.data_ptr(), d_rs.data_ptr(), True, s, slot)
        ix.dev_scan_counts(d_c.data_ptr(), n, d_ho.data_ptr(), d_scr.data_ptr(), s, slot)
        ix.dev_locate(d_rs.data_ptr(), d_ho.data_ptr(), n, total, d_g.data_ptr(), d_p.data_ptr(), s, slot, range_stride=1)
    outs = [("reads the packer refused", d_bad, np.zeros(1, np.uint64)), ("counts", d_c, np.diff(off)), ("hit offsets", d_ho, off),
            ("text positions", d_g, g), ("(record, offset) pairs", d_p, p)]
    return Job("pack + dev_count_nt2_long + scan + locate(stride 1) L=%d n=%d hits=%d" % (L, n, total), "nt", queue, outs,
               zeroed=(d_bad,), calls=4, heads=2, keep=(d_a, d_w, d_rs, d_scr))


def uniform_job(src, n, L, seed, alphabet=0):
    """dev_count_ascii_uniform; nucleotide batches carry N, lower case, 'u' and IUPAC letters"""
    q2d = _mix(src.text, n, L, seed, alphabet)
    if alphabet == 0:
        q2d = _dirty(q2d, seed)
    want = src.oi.parallel_count(*synth.fixed_to_csr(q2d), THREADS)[0]
    d_q, d_c, d_s = _up_bytes(q2d), _out(n), _out(n, "u1")

    def queue(ix, slot, s):
        ix.dev_count_ascii_uniform(d_q.data_ptr(), n, L, d_c.data_ptr(), d_s.data_ptr(), s, slot)
    return Job("dev_count_ascii_uniform %s L=%d n=%d" % ("aa" if alphabet else "nt", L, n), "aa" if alphabet else "nt", queue,
               [("counts", d_c, want), ("status", d_s, np.zeros(n, np.uint8))])


def locate_ascii_job(src, n, seed, alphabet=0):
    """dev_count_ascii_for_locate -> dev_scan_counts -> dev_locate (range stride 2) over queries of unequal lengths"""
    qb, qo = _ragged(src.text, n, 12, 41, seed, alphabet)
    off, g, p, _ = src.oi.parallel_locate(qb, qo, THREADS)
    total = int(off[-1])
    d_q, d_off = _up_bytes(qb), _up(qo)
    d_c, d_w, d_s, d_ho, d_g, d_p = _out(n), _out(2 * n), _out(n, "u1"), _out(n + 1), _out(total), _out(2 * total)
    d_scr = _out(src.ix.dev_scan_scratch_bytes(n) // 8 + 8)

    def queue(ix, slot, s):
        ix.dev_count_ascii_for_locate(d_q.data_ptr(), d_off.data_ptr(), n, d_c.data_ptr(), d_w.data_ptr(), d_s.data_ptr(), s, slot)
        ix.dev_scan_counts(d_c.data_ptr(), n, d_ho.data_ptr(), d_scr.data_ptr(), s, slot)
        ix.dev_locate(d_w.data_ptr(), d_ho.data_ptr(), n, total, d_g.data_ptr(), d_p.data_ptr(), s, slot, range_stride=2)
    outs = [("counts", d_c, np.diff(off)), ("status", d_s, np.zeros(n, np.uint8)), ("hit offsets", d_ho, off),
            ("text positions", d_g, g), ("(record, offset) pairs", d_p, p)]
    return Job("count_ascii_for_locate + scan + locate(stride 2) n=%d hits=%d" % (n, total), "aa" if alphabet else "nt", queue, outs,
               calls=3, heads=2, keep=(d_w, d_scr))


def mismatch_job(nt, n, L, k, seed):
    """dev_count_mismatch: counts per distance 0..k, from the variant-enumeration reference"""
    q2d = _mix(nt.text, n, L, seed)
    rng = np.random.default_rng(seed)
    q2d[np.arange(n), rng.integers(0, L, n)] = synth.NT[rng.integers(0, 4, n)]  # one letter redrawn: near misses of the text
    want, _ = mismatch_ref.oracle_counts_batch(nt.oi, [bytes(q) for q in q2d], k, 0, THREADS)
    qb, qo = synth.fixed_to_csr(q2d)
    d_q, d_off, d_c, d_s = _up_bytes(qb), _up(qo), _out(n * (k + 1)), _out(n, "u1")

    def queue(ix, slot, s):
        ix.dev_count_mismatch(d_q.data_ptr(), d_off.data_ptr(), n, k, d_c.data_ptr(), d_s.data_ptr(), s, slot)
    return Job("dev_count_mismatch k=%d L=%d n=%d" % (k, L, n), "nt", queue,
               [("counts per distance", d_c, want), ("status", d_s, np.zeros(n, np.uint8))], heads=1)


def ascii_job(src, n, seed, alphabet, lo=8, hi=31):
    """dev_count_ascii over queries of unequal lengths (amino batches of >= 4096: the k-mer schedule with per-query lengths)"""
    qb, qo = _ragged(src.text, n, lo, hi, seed, alphabet)
    want = src.oi.parallel_count(qb, qo, THREADS)[0]
    d_q, d_off, d_c, d_s = _up_bytes(qb), _up(qo), _out(n), _out(n, "u1")

    def queue(ix, slot, s):
        ix.dev_count_ascii(d_q.data_ptr(), d_off.data_ptr(), n, d_c.data_ptr(), None, d_s.data_ptr(), s, slot)
    return Job("dev_count_ascii %s n=%d" % ("aa" if alphabet else "nt", n), "aa" if alphabet else "nt", queue,
               [("counts", d_c, want), ("status", d_s, np.zeros(n, np.uint8))])


def heavy_job(nt, q2d, want):
    """the generic kernel over millions of 101-bp reads from the text, row intervals requested: no seed-and-verify, one LF
    step per letter -- tens of milliseconds, what the rest of a round is queued behind"""
    n, L = q2d.shape
    qb, qo = synth.fixed_to_csr(q2d)
    d_q, d_off, d_c, d_r = _up_bytes(qb), _up(qo), _out(n), _out(2 * n)

    def queue(ix, slot, s):
        ix.dev_count_ascii(d_q.data_ptr(), d_off.data_ptr(), n, d_c.data_ptr(), d_r.data_ptr(), None, s, slot)
    return Job("dev_count_ascii with row intervals, %d reads of %d bp" % (n, L), "nt", queue, [("counts", d_c, want)], keep=(d_r,))


# ------------------------------------------------------------------------------------------------------------------ fixtures

class Source:
    def __init__(self, text, st, hd, ix, oi):
        self.text, self.st, self.hd, self.ix, self.oi = text, st, hd, ix, oi


@pytest.fixture(scope="module")
def nt(oracle):
    """a repeat-rich nucleotide text (interspersed repeats, satellites, segmental duplications, N runs, 25 records): phase 2 and
    the left-context pass really receive survivors"""
    t0 = time.time()
    text, st, hd, _ = synth.repeat_rich_text(NT_TEXT, seed=23)
    oi = oracle.OracleIndex.from_text(text, 0, 8, 0, st, hd)
    t1 = time.time()
    ix = FmIndex.from_text(text, 0, 8, 0, st, hd).set_devices([0])
    print("[inflight] nucleotide text %d symbols: oracle index %.1f s, GPU index %.1f s, seed k %d, lcx %s"
          % (NT_TEXT, t1 - t0, time.time() - t1, ix.seed_kmer_len(), ix.lcx_enabled()))
    assert RUNG_L < ix.seed_kmer_len(), "the rung shape needs a seed table longer than its k-mers"
    return Source(text, st, hd, ix, oi)


@pytest.fixture(scope="module")
def aa(oracle):
    text, st, hd = synth.make_text(AA_TEXT, 1, 29, AA_RECORDS, 0.0)
    oi = oracle.OracleIndex.from_text(text, 1, 8, 0, st, hd)
    ix = FmIndex.from_text(text, 1, 8, 0, st, hd).set_devices([0])
    assert ix.seed_kmer_len() >= 1
    return Source(text, st, hd, ix, oi)


@pytest.fixture(scope="module")
def heavy_reads(nt):
    """HEAVY_N 101-bp reads from the text and the oracle's counts: the heavy first launch of a round and the read pool of the
    growth test"""
    t0 = time.time()
    q2d = _sampled_chunked(nt.text, HEAVY_N, HEAVY_L, 4000)
    want = nt.oi.parallel_count(*synth.fixed_to_csr(q2d), THREADS)[0]
    print("[inflight] oracle: %d reads of %d bp counted in %.1f s on %d threads" % (HEAVY_N, HEAVY_L, time.time() - t0, THREADS))
    return q2d, want


def stream_jobs(nt, aa, i):
    """every shape of a round for stream i: contents of its own (seeds), an order of its own (rotation + reversal)"""
    s = 1000 * (i + 1)
    jobs = []
    for j, L in enumerate((31, 32, 17)):
        for m, mode in enumerate((None, 1, 3)):
            jobs.append(kmer_job(nt, 40_000 + 1000 * i + 37 * j + m, L, s + 10 * j + m, mode))
    jobs.append(kmer_job(nt, 20_000 + 512 * i, RUNG_L, s + 50, None))  # below the seed k, n >= 4096: its own table ("rung")
    for j, L in enumerate((40, 101, 257)):
        jobs.append(reads_job(nt, 30_000 + 1000 * i + j, L, s + 60 + j))
    jobs.append(uniform_job(nt, 50_000 + 3 * i, 31, s + 70))
    jobs.append(uniform_job(nt, 50_000 + 5 * i, 101, s + 71))
    jobs.append(locate_ascii_job(nt, 20_000 + i, s + 80))
    jobs.append(mismatch_job(nt, 200 + i, 16, 1, s + 90))
    jobs.append(mismatch_job(nt, 200 + 2 * i, 16, 2, s + 91))
    jobs.append(uniform_job(aa, 50_000 + 7 * i, 12, s + 100, 1))
    jobs.append(uniform_job(aa, 30_000 + 7 * i, 40, s + 101, 1))
    jobs.append(ascii_job(aa, 20_000 + 11 * i, s + 102, 1))
    k = (5 * i + 3) % len(jobs)
    jobs = jobs[k:] + jobs[:k]
    return jobs[::-1] if i % 2 else jobs


@pytest.fixture(scope="module")
def jobsets(nt, aa):
    t0 = time.time()
    sets = [stream_jobs(nt, aa, i) for i in range(4)]
    print("[inflight] oracle: %d jobs for 4 streams prepared in %.1f s" % (sum(len(x) for x in sets), time.time() - t0))
    return sets


@pytest.fixture(scope="module")
def heavy(nt, heavy_reads):
    return heavy_job(nt, *heavy_reads)


_STREAMS = []  # every stream of the module stays alive: scratch is keyed by stream handle, and a "fresh" stream must be one


def _streams(n):
    """n new streams (at most four per test: the hardware queues a process gets)"""
    import torch
    assert n <= 4
    new = [torch.cuda.Stream() for _ in range(n)]
    _STREAMS.extend(new)
    return new


def _interleave(lists):
    """round-robin over the streams' job lists -> [(stream index, job)]"""
    out = []
    for k in range(max(len(x) for x in lists)):
        for si, x in enumerate(lists):
            if k < len(x):
                out.append((si, x[k]))
    return out


def run_round(idx, streams, lists, heavy_first=None, what="round"):
    """Warm-up (every shape once on its stream, then synchronise: scratch has grown, rungs exist), then the round proper:
    outputs re-filled with the sentinel, everything queued without a synchronise -- behind `heavy_first` on streams[0], whose
    completion event must still be pending when the last launch has been queued -- one synchronise, every output compared
    with the oracle.  -> (entry-point calls queued behind the event, seconds it took to queue them)"""
    import torch
    plan = _interleave(lists)
    for _, job in plan:
        job.reset()
    torch.cuda.synchronize()  # (the fills ran on torch's current stream)
    for si, job in plan:  # warm-up
        job.queue(idx, streams[si].cuda_stream, si)
    torch.cuda.synchronize()
    for _, job in plan:
        job.check(what + ", warm-up,")
        job.reset()
    if heavy_first is not None:
        heavy_first.reset()
    torch.cuda.synchronize()
    ev, calls = None, 0
    t0 = time.perf_counter()
    if heavy_first is not None:
        ev0, ev = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record(streams[0])
        heavy_first.queue(idx, streams[0].cuda_stream, 0)
        ev.record(streams[0])
    for si, job in plan:
        job.queue(idx, streams[si].cuda_stream, si)
        calls += job.calls
    pending = ev is not None and not ev.query()
    dt = time.perf_counter() - t0
    torch.cuda.synchronize()
    if heavy_first is not None:
        print("[inflight] %s: %d entry-point calls on %d streams queued in %.2f ms behind the first launch (which ran %.1f ms "
              "beside them); its event was %s" % (what, calls, len(streams), dt * 1e3, ev0.elapsed_time(ev),
                                                   "still pending" if pending else "ALREADY COMPLETE"))
        assert pending, ("%s: the first launch had finished before the last one was queued (%d calls, %.2f ms): nothing was "
                         "in flight across streams, so this run shows nothing about it" % (what, calls, dt * 1e3))
        heavy_first.check(what + ",")
    for si, job in plan:
        job.check("%s, stream %d," % (what, si))
    return calls, dt


class lcx_off:
    """the index without its left-context index (reads then take count_nt2_reads_kernel over per-block lists)"""

    def __init__(self, ix):
        self.ix = ix

    def __enter__(self):
        self.ix.set_lcx(False)
        assert not self.ix.lcx_enabled()

    def __exit__(self, *exc):
        self.ix.set_lcx(True)


# ------------------------------------------------------------------------------------------------------------------ test 1

@pytest.mark.parametrize("lcx", [True, False], ids=["lcx", "no_lcx"])
def test_four_streams_everything_queued_before_anything_finishes(nt, aa, jobsets, heavy, lcx):
    """Steady state: after a warm-up round, every shape -- k-mers in the policy mode and in modes 1 and 3, the rung, reads of
    40 / 101 / 257 bp with range starts into locate (stride 1), the uniform entry point with N / lower case / IUPAC, the
    ASCII locate pipeline (stride 2), mismatch counts for k = 1, 2, amino uniform 12 / 40 and ragged amino -- is queued on each
    of four streams without a synchronise, each stream with data, buffers and an order of its own.  The first launch on
    the first stream is the generic kernel over three million 101-bp reads; its event must still be pending once the last
    launch is queued (the test fails, not skips, when it is not).  Once with the left-context index resident (reads take the
    pooled pass and its device-wide LF list), once without it."""
    assert nt.ix.lcx_enabled(), "the default policy keeps the left-context index resident on this index"
    idx = {"nt": (nt.ix, 0), "aa": (aa.ix, 0)}
    streams = _streams(4)
    if lcx:
        run_round(idx, streams, jobsets, heavy, "four streams, left-context index resident")
    else:
        with lcx_off(nt.ix):
            run_round(idx, streams, jobsets, heavy, "four streams, no left-context index")


def test_first_use_of_a_rung_while_other_streams_are_busy(nt, heavy_reads):
    """The first batch of >= 4096 k-mers of a length below the seed k builds that length's table inside the call.  Three
    streams are given long launches first; the fourth then asks for a length nobody has asked for.  (The build is synchronous
    and frees its scratch, which waits for the device: whether the other launches are still running when it returns is the
    runtime's business, so no in-flight condition is asserted here -- the steady-state rung launch is part of the round
    above, which asserts it.)"""
    import torch
    L = RUNG_L + 1
    assert L < nt.ix.seed_kmer_len()
    q2d, want = heavy_reads
    idx = {"nt": (nt.ix, 0)}
    streams = _streams(4)
    busy = [heavy_job(nt, q2d[a:a + 400_000], want[a:a + 400_000]) for a in (0, 700_000, 1_400_000)]
    rung = [kmer_job(nt, 30_000 + 999 * j, L, 7000 + j, None) for j in range(2)]
    for j in busy + rung:
        j.reset()
    torch.cuda.synchronize()
    for j, s in zip(busy, streams):
        j.queue(idx, s.cuda_stream)
    rung[0].queue(idx, streams[3].cuda_stream)  # builds the table
    rung[1].queue(idx, streams[0].cuda_stream)  # finds it
    torch.cuda.synchronize()
    for j in busy + rung:
        j.check("first use of a rung,")


# ------------------------------------------------------------------------------------------------------------------ test 2

class Pool:
    """one scratch user of the growth test: a pool of GROWTH_SIZES[-1] queries on the device, the oracle's counts of all of
    them, and launch(ix, first query, n, d_counts, stream) over any slice"""

    def __init__(self, name, which, want, launch, keep):
        self.name, self.which, self.want, self.launch, self.keep = name, which, want, launch, keep


@pytest.fixture(scope="module")
def pools(nt, aa, heavy_reads):
    import torch
    N = GROWTH_SIZES[-1]
    t0 = time.time()
    out = {}
    # k-mers, two-phase schedule (mode 3 pinned: the policy's choice for this index, whatever the seed k)
    q = _mix(nt.text, N, 31, 5001)
    d_kw = _up(_pack_words(q))

    def kmers(ix, a, n, d_c, s):
        _lib().awry_debug_set_count_kernel(3)
        try:
            ix.dev_count_nt2(d_kw.data_ptr() + 8 * a, n, 31, d_c.data_ptr(), True, s, 0)
        finally:
            _lib().awry_debug_set_count_kernel(-1)
    out["kmers"] = Pool("two-phase 31-mers", "nt", nt.oi.parallel_count(*synth.fixed_to_csr(q), THREADS)[0], kmers, (d_kw,))
    # 101-bp reads, packed once; the launches are dev_count_nt2_long over slices of the words
    r2d, rwant = heavy_reads
    d_ra, d_rw, d_bad = _up_bytes(r2d), _out(N * 4), _out(1)
    d_bad.zero_()
    nt.ix.dev_pack_nt2(d_ra.data_ptr(), N, HEAVY_L, d_rw.data_ptr(), d_bad.data_ptr(), None, 0)
    torch.cuda.synchronize()
    assert int(d_bad[0]) == int(((r2d == ord("N")).any(axis=1)).sum())
    clean = ~(r2d == ord("N")).any(axis=1)  # (reads with N are not packable: their counts are not compared)
    del d_ra

    def reads(ix, a, n, d_c, s):
        ix.dev_count_nt2_long(d_rw.data_ptr() + 32 * a, n, HEAVY_L, d_c.data_ptr(), None, True, s, 0)
    out["reads"] = Pool("two-phase 101-bp reads", "nt", rwant, reads, (d_rw,))
    out["reads"].clean = clean
    # the uniform entry point on the nucleotide index (packs into u_words, lists what it cannot pack)
    q = _dirty(_mix(nt.text, N, 40, 5003), 5004)
    d_uq = _up_bytes(q)

    def uniform(ix, a, n, d_c, s):
        ix.dev_count_ascii_uniform(d_uq.data_ptr() + 40 * a, n, 40, d_c.data_ptr(), None, s, 0)
    out["uniform"] = Pool("uniform entry point, 40 bp", "nt", nt.oi.parallel_count(*synth.fixed_to_csr(q), THREADS)[0], uniform, (d_uq,))
    # amino 12-mers, the amino two-phase schedule
    q = _mix(aa.text, N, 12, 5005, 1)
    d_aq = _up_bytes(q)

    def amino(ix, a, n, d_c, s):
        ix.dev_count_ascii_uniform(d_aq.data_ptr() + 12 * a, n, 12, d_c.data_ptr(), None, s, 0)
    out["amino"] = Pool("amino 12-mers", "aa", aa.oi.parallel_count(*synth.fixed_to_csr(q), THREADS)[0], amino, (d_aq,))
    print("[inflight] oracle: growth pools of %d queries (31-mers, 40-bp, amino 12-mers) counted in %.1f s" % (N, time.time() - t0))
    return out


# first query of each launch (multiples of 8, so that every slice of bytes starts on an 8-byte boundary), per stream
GROWTH_FIRST = ((16, 999_992, 2_500_000, 0), (1_000_000, 0, 40, 64))


def _growth(pool, ix, streams):
    """GROWTH_SIZES queued back to back on each stream (interleaved over the streams), fresh streams: scratch is first
    allocated, grown, kept, grown again while earlier launches of that stream -- and of the other -- are queued"""
    import torch
    N = GROWTH_SIZES[-1]
    launches = []
    for k, size in enumerate(GROWTH_SIZES):
        for si in range(len(streams)):
            a = GROWTH_FIRST[si][k]
            n = min(size, N - a)
            launches.append((si, a, n, _out(n)))
    for _, _, _, d_c in launches:
        d_c.fill_(SENT)
    torch.cuda.synchronize()
    # two launches of a stream, then two of the next: the second stream allocates and grows while the first has work queued
    order = sorted(range(len(launches)), key=lambda j: (j // (2 * len(streams)), launches[j][0], j))
    for j in order:
        si, a, n, d_c = launches[j]
        pool.launch(ix, a, n, d_c, streams[si].cuda_stream)
    torch.cuda.synchronize()
    mask = getattr(pool, "clean", None)
    for si, a, n, d_c in launches:
        got, want = d_c[:n].cpu().numpy().view(np.uint64), pool.want[a:a + n]
        if mask is not None:
            got, want = got[mask[a:a + n]], want[mask[a:a + n]]
        bad = np.flatnonzero(got != want)
        assert len(bad) == 0, "%s, stream %d, queries [%d, %d): %d counts differ from the oracle, first at %d: got %#x, expected %d" % (
            pool.name, si, a, a + n, len(bad), bad[0], int(got[bad[0]]), int(want[bad[0]]))


@pytest.mark.parametrize("nstreams", [1, 2])
@pytest.mark.parametrize("user", ["kmers", "reads_lf_list", "reads_block_lists", "uniform", "amino"])
def test_scratch_grows_while_work_is_queued(nt, aa, pools, user, nstreams):
    """One shape at 5 000 -> 2 000 003 -> 63 -> 3 000 001 queries on one stream without a synchronise in between, for every
    user of per-stream scratch; then the same on two fresh streams at once."""
    streams = _streams(nstreams)
    if user == "reads_lf_list":
        assert nt.ix.lcx_enabled()
        _growth(pools["reads"], nt.ix, streams)
    elif user == "reads_block_lists":
        with lcx_off(nt.ix):
            _growth(pools["reads"], nt.ix, streams)
    else:
        p = pools[user]
        _growth(p, aa.ix if p.which == "aa" else nt.ix, streams)


# ------------------------------------------------------------------------------------------------------------------ test 3

@pytest.fixture(scope="module")
def ring(oracle):
    """a smaller index without the seed-and-verify accelerators: locate then walks (tile pass + walk pass: two heads per call)"""
    text, st, hd = synth.make_text(1_000_000, 0, 41, 4, 0.02)
    oi = oracle.OracleIndex.from_text(text, 0, 8, 0, st, hd)
    ix = FmIndex.from_text(text, 0, 8, 0, st, hd).set_devices([0])
    ix.set_verify(-1)           # (the default policy keeps the ratio-1 dense SA resident: back to the file's samples)
    ix.set_locate_sa_ratio(0)
    assert not ix.verify_enabled() and ix.locate_sa_ratio() == 8
    src = Source(text, st, hd, ix, oi)
    q2d = _sampled_chunked(text, 1_500_000, 101, 77)
    src.blocker = heavy_job(src, q2d, oi.parallel_count(*synth.fixed_to_csr(q2d), THREADS)[0])
    return src


def ring_jobs(src, i):
    s = 300 * (i + 1)
    return [locate_ascii_job(src, 9_000 + i, s), mismatch_job(src, 150 + i, 14, 1, s + 1), kmer_job(src, 30_000 + i, 31, s + 2, 1),
            locate_ascii_job(src, 7_000 + i, s + 3), mismatch_job(src, 120 + i, 14, 2, s + 4), kmer_job(src, 20_000 + i, 24, s + 5, 1),
            reads_job(src, 8_000 + i, 50, s + 6), kmer_job(src, 10_000 + i, 32, s + 7, 1)]


@pytest.mark.parametrize("nstreams", [1, 2])
def test_head_ring_wraps_while_earlier_launches_are_queued(ring, nstreams):
    """Locate (two heads each), mismatch and the chunk kernel (one each) queued on one stream without a synchronise: eleven
    heads from a ring of eight per stream, behind a long first launch so that the early ones are still queued when the ring
    comes back to their heads.  Once on one stream, once interleaved over two."""
    lists = [ring_jobs(ring, i) for i in range(nstreams)]
    for x in lists:
        assert sum(j.heads for j in x) >= 9 and len(x) >= 8
    run_round({"nt": (ring.ix, 0)}, _streams(nstreams), lists, ring.blocker, "head ring, %d stream(s)" % nstreams)


# ------------------------------------------------------------------------------------------------------------------ test 4

def test_host_threads_mixed_with_streams(nt, aa, jobsets):
    """Four Python threads, each with a stream of its own, run the device-resident round three times; meanwhile two more
    threads call the host batch and scalar entry points the existing thread test omits: mismatch count / locate, packed
    k-mers, count_string / locate_string / search_range (the mailbox), and amino count / locate of 30 000 queries of unequal
    lengths (the generic pipelined lanes).  (The count-kernel mode is a process-wide switch and every mode gives the same
    counts; with several threads flipping it, which schedule a launch takes is not fixed -- its answer is.)"""
    import torch
    idx = {"nt": (nt.ix, 0), "aa": (aa.ix, 0)}
    streams = _streams(4)
    # host-side work and what the oracle says, before anything starts
    mq = _mix(nt.text, 120, 18, 8101)
    mqb, mqo = synth.fixed_to_csr(mq)
    m_c, _, m_off, m_g, m_p, m_d = mismatch_ref.oracle_search_batch(nt.oi, [bytes(q) for q in mq], 1, 0, THREADS, True)
    pk = _mix(nt.text, 100_000, 31, 8102)
    pk_words, pk_want = _pack_words(pk), nt.oi.parallel_count(*synth.fixed_to_csr(pk), THREADS)[0]
    singles = [bytes(q) for L in (5, 12, 31, 60) for q in _mix(nt.text, 6, L, 8103 + L)]
    s_count = [nt.oi.count_string(q) for q in singles]
    s_loc = [nt.oi.locate_string(q) for q in singles]
    s_rng = [nt.oi.search_range(q) for q in singles]
    aqb, aqo = _ragged(aa.text, 30_000, 4, 24, 8104, 1)
    lens = np.diff(aqo.astype(np.int64))
    assert lens.min() >= 1
    a_off, a_g, a_p, _ = aa.oi.parallel_locate(aqb, aqo, THREADS)
    for x in jobsets:
        for j in x:
            j.reset()
    torch.cuda.synchronize()
    errors, lock = [], threading.Lock()

    def guarded(fn):
        def run(*a):
            try:
                fn(*a)
            except BaseException as e:  # noqa: BLE001
                import traceback
                with lock:
                    errors.append((fn.__name__, a[:1], repr(e), traceback.format_exc()))
        return run

    @guarded
    def device_thread(i):
        torch.cuda.set_device(0)
        for rnd in range(3):
            for j in jobsets[i]:
                j.queue(idx, streams[i].cuda_stream)
            streams[i].synchronize()
            with torch.cuda.stream(streams[i]):  # this thread's copies and fills stay on its own stream
                for j in jobsets[i]:
                    j.check("thread %d, round %d," % (i, rnd))
                    j.reset()
            streams[i].synchronize()

    @guarded
    def host_nt_thread():
        for rnd in range(3):
            assert np.array_equal(nt.ix.parallel_count_mismatch_csr(mqb, mqo, 1), m_c), rnd
            off, g, p, d = nt.ix.parallel_locate_mismatch_csr(mqb, mqo, 1)
            assert np.array_equal(off, m_off) and np.array_equal(g, m_g) and np.array_equal(p, m_p) and np.array_equal(d, m_d), rnd
            assert np.array_equal(nt.ix.parallel_count_packed(pk_words, 31), pk_want), rnd
            for q, c, (lg, lp), (sp, ep) in zip(singles, s_count, s_loc, s_rng):
                assert nt.ix.count_string(q) == c, (rnd, q)
                g, p = nt.ix.locate_string_raw(q)
                assert np.array_equal(g, lg) and [tuple(int(v) for v in r) for r in p] == lp, (rnd, q)
                r = nt.ix.search_range(q)
                assert (r.start_ptr, r.end_ptr) == (sp, ep), (rnd, q)

    @guarded
    def host_aa_thread():
        for rnd in range(3):
            assert np.array_equal(aa.ix.parallel_count_csr(aqb, aqo), np.diff(a_off)), rnd
            off, g, p = aa.ix.parallel_locate_csr(aqb, aqo)
            assert np.array_equal(off, a_off) and np.array_equal(g, a_g) and np.array_equal(p, a_p), rnd

    threads = [threading.Thread(target=device_thread, args=(i,)) for i in range(4)]
    threads += [threading.Thread(target=host_nt_thread), threading.Thread(target=host_aa_thread)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    _lib().awry_debug_set_count_kernel(-1)
    assert not errors, "\n".join("%s%s: %s\n%s" % e for e in errors)


# ------------------------------------------------------------------------------------------------------------------ test 5

def test_two_replicas_on_one_gpu(nt, aa, jobsets, heavy):
    """set_devices([0, 0]) with a small seed table: the round with two streams on slot 0 and two on slot 1 at once (each
    replica keeps scratch, rungs and heads of its own), then a sharded parallel_count."""
    ix2 = FmIndex.from_text(nt.text, 0, 8, 0, nt.st, nt.hd)
    ix2.set_seed_kmer_len(11)
    ix2.set_devices([0, 0])
    assert ix2.num_devices() == 2 and ix2.seed_kmer_len() == 11 and RUNG_L < 11
    streams = _streams(4)

    def idx(which, si):  # streams 0, 1 -> replica 0; streams 2, 3 -> replica 1 (the amino shapes stay on their own index)
        return (aa.ix, 0) if which == "aa" else (ix2, 0 if si < 2 else 1)
    run_round(idx, streams, jobsets, heavy, "two replicas on one GPU, two streams each")
    qb, qo = _ragged(nt.text, 100_000, 1, 70, 9100)
    assert np.array_equal(ix2.parallel_count_csr(qb, qo), nt.oi.parallel_count(qb, qo, THREADS)[0])
    q2d = _mix(nt.text, 200_000, 31, 9101)  # (a shard of >= 65 536 fixed-length queries: the host-packed lanes of each replica)
    qb, qo = synth.fixed_to_csr(q2d)
    assert np.array_equal(ix2.parallel_count_csr(qb, qo), nt.oi.parallel_count(qb, qo, THREADS)[0])


# ------------------------------------------------------------------------------------------------------------------ test 6

def test_wide_rows_two_streams(nt, jobsets):
    """The wide-row kernels (64-bit rows) under count-kernel mode 3 use the same per-stream lists (two_phase_lists): k-mers
    and packed reads on two streams at once."""
    L_ = _lib()
    L_.awry_debug_force_wide_rows(1)
    try:
        try:
            wx = FmIndex.from_text(nt.text, 0, 8, 0, nt.st, nt.hd).set_devices([0])
        finally:
            L_.awry_debug_force_wide_rows(0)
        assert "count_nt2_wide_kernel" in wx.count_schedule(31) and wx.seed_kmer_len() >= 1
        L_.awry_debug_set_count_kernel(3)
        assert "count_nt2_wide_probe_kernel" in wx.count_schedule(31)
        lists = []
        for i in range(2):
            mine = [j for j in jobsets[i] if j.name.startswith("pack + dev_count_nt2_long") or "mode=None" in j.name]
            assert len(mine) >= 6
            lists.append(mine)
        import torch
        streams = _streams(2)
        idx = {"nt": (wx, 0)}
        plan = _interleave(lists)
        for rnd in range(2):  # first use (scratch grows), then steady state
            for _, j in plan:
                j.reset()
            torch.cuda.synchronize()
            for si, j in plan:
                j.queue(idx, streams[si].cuda_stream)
            torch.cuda.synchronize()
            for si, j in plan:
                j.check("wide rows, round %d, stream %d," % (rnd, si))
    finally:
        L_.awry_debug_force_wide_rows(0)
        L_.awry_debug_set_count_kernel(-1)


# ------------------------------------------------------------------------------------------------------------------ part B

def test_generic_host_drivers_in_a_child_process(oracle, tmp_path):
    """AWRY_HOST_PATH=generic is read once per process, so the unpipelined host drivers (count_shard_generic,
    locate_shard_generic) run in a fresh child: parallel_count_csr / parallel_locate_csr of 6 000 fixed-length nucleotide
    queries (clean, and with N / 'u' / lower case / IUPAC) and of 8 192 amino 12-mers (the amino two-phase schedule on the
    replica's own stream), from one thread and then from four threads at once.  The child writes what it got; the oracle's
    answers are computed here.  AWRY_TRACE_HOST=1 proves which drivers ran: both batch entry points report, and neither
    pipelined path (host-packed shard, generic shard, packed locate shard) does."""
    from tests import _generic_host_worker as w
    # (AWRY_PREWARM=0: awry_set_devices would otherwise warm the packed lanes with one real host-packed call, and trace it)
    env = dict(os.environ, AWRY_HOST_PATH="generic", AWRY_TRACE_HOST="1", AWRY_PREWARM="0")
    out = str(tmp_path)
    proc = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.join(ROOT, "tests", "_generic_host_worker.py"), out],
                          env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert proc.returncode == 0, "worker exited with %d\n%s\n%s" % (proc.returncode, proc.stdout[-2000:], proc.stderr[-4000:])
    err = proc.stderr
    assert "[awry] awry_count_batch" in err and "[awry] awry_locate_batch" in err, "the trace is missing: " + err[-2000:]
    for line in ("generic shard", "host-packed shard", "packed locate shard"):
        assert line not in err, "a pipelined driver ran in the child (%s): the knob did not take effect" % line
    checked = 0
    for name, alphabet, text, st, hd, batches in w.cases():
        oi = oracle.OracleIndex.from_text(text, alphabet, 8, 0, st, hd)
        for who in w.callers():
            for bname, qb, qo in batches[who]:
                off, g, p, _ = oi.parallel_locate(qb, qo, THREADS)
                got = {a: np.load(os.path.join(out, "%s_%s_%s_%s.npy" % (name, bname, who, a))) for a in ("counts", "off", "gpos", "pos")}
                assert np.array_equal(got["counts"], np.diff(off)), (name, bname, who)
                assert np.array_equal(got["off"], off) and np.array_equal(got["gpos"], g) and np.array_equal(got["pos"], p), (name, bname, who)
                checked += 1
    assert checked == 3 * (1 + w.NTHREADS)
