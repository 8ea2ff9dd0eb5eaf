"""Substitution-tolerant count and locate at the batch sizes they are meant for (tests/test_mismatch_gpu.py checks the
semantics on batches of a few hundred queries): lanes that search many queries one after the other, the segmented sort of
the leaves in its partitioned regime with small, medium and large segments, batches that cross the chunk cuts of
chunk_queries (2^24 queries, 2^29 query bytes), two replicas, and a wide-row (64-bit) replica.

The device of every case is a verified POOL and a drawn BATCH.  The pool is a few hundred distinct queries per index
(a 3 Mbp nucleotide text and a 1e6-residue amino text, several records, N / X runs) whose counts[k + 1] come from the
variant-enumeration reference (mismatch_ref.oracle_counts_batch) and whose hit lists, in the promised order, come from
mismatch_ref.oracle_search_batch; test_pool_is_the_definition shows both equal to the brute-force definition and to
mismatch_ref.oracle_locate on a subset of every class.  A batch is millions of draws from the pool with replacement in a
seeded order and its expected result is the pool's result gathered by draw index, so a lane meets a random sequence of long,
short, leafless, heavy and rejected queries and a result that depends on what the lane did before differs from a value
verified on its own.  Every comparison is exact equality of integers; every condition on the inputs (n >= 8 x resident
lanes, class shares, rows next to a cut drawn from the pool, the hit budget) is asserted from the reference's numbers.

HIT_BUDGET = 2^25 hits per located batch is a host-memory guard (a hit costs 25 bytes in the result arrays, and as much
again in the expected ones), not a tolerance.  A pool entry is located only when its k = 2 total is at most
LOCATE_MAX = HIT_BUDGET / 256 hits, so that no single entry takes more than 1/256 of a batch's budget.

Wall times on one MI355X (256 CUs) inside one `pytest -m gpu` run of 357 s (each test also prints its own): this file 38 s.
Pool references (fixture) 6.9 s nucleotide + 3.1 s amino, pool checks 1.3 / 0.6 s, lane refill count 2.7 / 7.4 s (n = 4 456 448;
the k = 2 device call itself 0.34 / 1.94 s), lane refill locate 1.9 / 5.1 s (n = 2 097 152, 8.1 M / 7.7 M hits at k = 2), sort
regimes 5.0 s (0.27 s the call, 4.4 s with the capacity at 1/16), chunk cuts 0.7 s (17.8 M 12-mers), 0.4 s (5.5 M reads) and
2.4 s (17.0 M 20-mers located), wide rows 0.3 s.  The parent commit's `pytest -m gpu` was not measured on that machine; the last recorded
whole-suite run before this file (GPUTEST_r03.json, an older commit) is 150 passed in 218 s."""
import time

import numpy as np
import pytest

from awry_amd.fm_index import FmIndex, pack_queries
from tests import mismatch_ref as mr
from tests import synth

pytestmark = pytest.mark.gpu

THREADS = 16
HIT_BUDGET = 1 << 25
LOCATE_MAX = HIT_BUDGET >> 8
LANES_PER_CU = 2048            # 8 waves x 4 SIMDs x 64 lanes: the ceiling on resident lanes per CU whatever the kernel's registers
MAXQ, MAXB = 1 << 24, 1 << 29  # chunk_queries (host_count.h)
REJECTED = ((b"", 1), (b"AC$T", 2), (b"A#C", 2), (b"$", 2), (bytes([0x41, 0x80, 0x47]), 3), (bytes([0x24, 0xFF]), 3))  # (query, status)


def chunk_cuts(qo):
    """the chunks chunk_queries makes of a whole batch -> [(lo, hi)]"""
    out, a, hi = [], 0, len(qo) - 1
    while a < hi:
        b = min(hi, a + MAXQ)
        while b > a + 1 and int(qo[b]) - int(qo[a]) > MAXB:
            b = a + (b - a) // 2
        out.append((a, b))
        a = b
    return out


def gather(off, draw, *arrays):
    """CSR rows `draw` (with repeats) of (off, arrays) -> (offsets of the gathered batch, each array's entries in that order)"""
    start = off[:-1].astype(np.int64)[draw]
    lens = np.diff(off.astype(np.int64))[draw]
    o = np.zeros(len(draw) + 1, np.uint64)
    o[1:] = np.cumsum(lens)
    outs = [np.empty((int(o[-1]),) + a.shape[1:], a.dtype) for a in arrays]
    step = 1 << 20
    for a in range(0, len(draw), step):
        e = min(len(draw), a + step)
        lo, hi = int(o[a]), int(o[e])
        src = np.repeat(start[a:e] - o[a:e].astype(np.int64), lens[a:e]) + np.arange(lo, hi)
        for dst, arr in zip(outs, arrays):
            dst[lo:hi] = arr[src]
    return (o,) + tuple(outs)


def keep_within(loc, k):
    """the hit lists at <= k substitutions from the lists at <= 2: the hits of distance <= k, in the same (row) order"""
    off, g, p, d = loc
    seg = np.repeat(np.arange(len(off) - 1), np.diff(off.astype(np.int64)))
    keep = d <= k
    o = np.zeros(len(off), np.uint64)
    o[1:] = np.cumsum(np.bincount(seg[keep], minlength=len(off) - 1))
    return o, g[keep], p[keep], d[keep]


def plant(q2d, nsub, rng, alphabet):
    """nsub substitutions per query at distinct random columns, each to another letter"""
    abc = synth.NT if alphabet == 0 else synth.AA
    out = q2d.copy()
    for r in range(len(out)):
        for c in rng.choice(out.shape[1], size=min(nsub, out.shape[1]), replace=False):
            j = int(np.searchsorted(abc, out[r, c]))
            j = j if j < len(abc) and abc[j] == out[r, c] else 0
            out[r, c] = abc[(j + int(rng.integers(1, len(abc)))) % len(abc)]
    return out


def pool_queries(text, st, alphabet, rng):
    """-> [(class name, query bytes)], distinct"""
    out, seen = [], set()

    def add(cls, qs):
        for q in qs:
            q = bytes(q)
            if q not in seen:
                seen.add(q)
                out.append((cls, q))

    def four(L, n, tag="", seed=0):
        s = synth.sampled_queries(text, n, L, 1000 * L + seed, alphabet=alphabet)
        add("sampled" + tag, s)
        add("planted1" + tag, plant(s, 1, rng, alphabet))
        add("planted2" + tag, plant(s, 2, rng, alphabet))
        add("random" + tag, synth.random_queries(n, L, alphabet, 2000 * L + seed))

    amb = ord("N") if alphabet == 0 else ord("X")
    if alphabet == 0:
        for L in list(range(1, 41)) + [45, 50, 56, 64]:
            four(L, 1)
        for L in (65, 80, 101, 120):
            four(L, 1, "_long")
        four(12, 40, "_12", 1)    # the fixed-length sets of the chunk cases
        four(20, 100, "_20", 1)
        four(101, 15, "_101", 1)
        four(31, 30, "", 1)
        four(10, 10, "", 1)
        four(11, 10, "", 1)
        odd = [b"ACGTRYKMSWBDHVN", b"acgtnnnnacgt", b"NNNN", b"N", b"u", b"nACGTn"]
    else:
        for L in list(range(1, 13)) + [16, 20, 31, 40]:
            four(L, 1)
        s = synth.sampled_queries(text, 4, 64, 64, alphabet=1)
        add("sampled_long", s[:1])
        add("planted1_long", plant(s[1:2], 1, rng, 1))
        add("planted2_long", plant(synth.sampled_queries(text, 1, 80, 80, alphabet=1), 2, rng, 1))
        add("sampled_long", synth.sampled_queries(text, 1, 120, 120, alphabet=1))
        add("random_long", synth.random_queries(1, 70, 1, 70))
        add("random", synth.random_queries(10, 3, 1, 3))     # the segment classes of the sort case: 3- and 4-mers have
        add("random", synth.random_queries(40, 4, 1, 4))     # more than 1 000 occurring variants at k = 2, 5- and 6-mers
        add("random", synth.random_queries(20, 5, 1, 5))     # hundreds, random 8- and 12-mers mostly none
        add("random", synth.random_queries(60, 6, 1, 6))
        add("random", synth.random_queries(80, 8, 1, 8))
        add("random", synth.random_queries(40, 12, 1, 12))
        for L in (8, 9, 10, 12):
            four(L, 15, "", 1)
        odd = [b"mkvB", b"ACGU", b"XXX", b"x", b"BZJOU", b"MKVLXAAG"]
    n = len(text) - 1
    joins = [bytes(text[s - 6:s + 9]) for s in st[1:]] + [bytes(text[s - 20:s + 11]) for s in st[1:3]] + [bytes(text[s - 2:s + 1]) for s in st[1:3]]
    add("join", joins)
    run = np.flatnonzero(text[:-1] == amb)
    p = int(run[len(run) // 2])
    add("amb_run", [bytes(text[max(0, p - 10):p + 10]), bytes(text[int(run[0]) - 8:int(run[0]) + 4]), bytes(text[int(run[-1]) - 2:int(run[-1]) + 9])])
    p = int(rng.integers(0, n - 30))
    w = bytes(text[p:p + 30])
    add("disguised", [w.lower(), w.replace(b"T", b"U") if alphabet == 0 else w.replace(b"A", b"a"), w.replace(b"A", b"R" if alphabet == 0 else b"B", 2)] + odd)
    return out


class World:
    """one index, its oracle, its verified pool"""

    def __init__(self, oracle, alphabet):
        t0 = time.time()
        self.alphabet = alphabet
        if alphabet == 0:
            self.text, self.st, self.hd = synth.make_text(3_000_000, 0, 0x5CA1E, 6, 0.01)
        else:
            self.text, self.st, self.hd = synth.make_text(1_000_000, 1, 0x5CA1F, 8, 0.005)
        self.ix = FmIndex.from_text(self.text, alphabet, 8, 0, self.st, self.hd).set_devices([0])
        self.oi = oracle.OracleIndex.from_text(self.text, alphabet, 8, 0, self.st, self.hd)
        cq = pool_queries(self.text, self.st, alphabet, np.random.default_rng(77 + alphabet))
        self.cls = np.array([c for c, _ in cq])
        self.q = [q for _, q in cq]
        self.P = len(self.q)
        self.qb, self.qo = pack_queries(self.q)
        self.len = np.diff(self.qo.astype(np.int64))
        self.counts, self.leaves = mr.oracle_counts_batch(self.oi, self.q, 2, alphabet, THREADS)  # the k result: columns 0 .. k
        self.tot = {k: self.counts[:, :k + 1].sum(axis=1).astype(np.int64) for k in (0, 1, 2)}
        self.loc_ok = np.flatnonzero(self.tot[2] <= LOCATE_MAX)
        self.loc_row = np.full(self.P, -1, np.int64)          # pool entry -> row of the located subset
        self.loc_row[self.loc_ok] = np.arange(len(self.loc_ok))
        r = mr.oracle_search_batch(self.oi, [self.q[i] for i in self.loc_ok], 2, alphabet, THREADS, True)
        assert np.array_equal(r[0], self.counts[self.loc_ok]) and np.array_equal(r[1], self.leaves[self.loc_ok])
        self.loc = {2: r[2:]}
        for k in (0, 1):
            self.loc[k] = keep_within(r[2:], k)
            assert np.array_equal(np.diff(self.loc[k][0].astype(np.int64)), self.tot[k][self.loc_ok])
        self.setup_s = time.time() - t0
        print("pool (alphabet %d): %d queries, lengths 1..%d, %d located (%d reference hits), max leaves %d, setup %.1f s"
              % (alphabet, self.P, int(self.len.max()), len(self.loc_ok), len(r[3]), int(self.leaves.max()), self.setup_s))

    def close(self):
        self.ix.close()
        self.oi.close()

    def draw_weights(self, entries, long_share=0.03):
        """probabilities over `entries`: uniform, with the queries longer than 64 held to long_share of the draws (k = 2 on
        them costs ten times a 31-mer)"""
        w = np.ones(len(entries))
        lng = self.len[entries] > 64
        if lng.any() and not lng.all():
            w[lng] = long_share / (1 - long_share) * (~lng).sum() / lng.sum()
        return w / w.sum()

    def batch_bytes(self, draw):
        o, b = gather(self.qo, draw, self.qb)
        return b, o


@pytest.fixture(scope="module")
def worlds(oracle):
    """both worlds (0 nucleotide, 1 amino) for the module; the replicas and the oracle indexes are released at its end"""
    w = {}
    try:
        for alphabet in (0, 1):
            w[alphabet] = World(oracle, alphabet)
        yield w
    finally:
        for x in w.values():
            x.close()


both_alphabets = pytest.mark.parametrize("alphabet", [0, 1], ids=["nucleotide", "amino"])


def resident_lanes():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count * LANES_PER_CU


def locate_equals(got, want, what):
    for name, x, y in zip(("offsets", "positions", "(record, offset)", "distances"), got, want):
        assert x.shape == y.shape and np.array_equal(x, y), (what, name)


@both_alphabets
def test_pool_is_the_definition(worlds, alphabet):
    """the pool's expected values on a subset of every class: counts against brute force over the text, hit lists against
    brute force as sets and against mismatch_ref.oracle_locate in order, for k = 0, 1, 2"""
    t0 = time.time()
    w = worlds[alphabet]
    assert 300 <= w.P <= 2000 and int(w.len.min()) == 1 and int(w.len.max()) == 120
    subset = []
    for c in np.unique(w.cls):
        subset += list(np.flatnonzero(w.cls == c)[:2])
    for L in (1, 2, 3, 12, 20):
        subset += list(np.flatnonzero(w.len == L)[:2])
    subset = sorted(set(int(i) for i in subset))
    located = 0
    for i in subset:
        want, pos, dist = mr.brute_force(w.text, w.q[i], 2, w.alphabet)
        assert np.array_equal(w.counts[i], want), (w.q[i], w.counts[i], want)
        if w.loc_row[i] < 0:
            continue
        located += 1
        for k in (0, 1, 2):
            off, g, p, d = w.loc[k]
            a, b = int(off[w.loc_row[i]]), int(off[w.loc_row[i] + 1])
            order = np.argsort(g[a:b], kind="stable")
            assert np.array_equal(g[a:b][order].astype(np.int64), pos[dist <= k]) and np.array_equal(d[a:b][order], dist[dist <= k]), (w.q[i], k)
            if b - a <= 4096 and len(w.q[i]) <= 40:
                og, op, od = mr.oracle_locate(w.oi, w.q[i], k, w.alphabet)
                assert np.array_equal(g[a:b], og) and np.array_equal(p[a:b], op) and np.array_equal(d[a:b], od), (w.q[i], k)
    assert located >= len(subset) // 2
    print("pool check (alphabet %d): %d entries against brute force, %d of them located, %.1f s" % (w.alphabet, len(subset), located, time.time() - t0))


@both_alphabets
def test_lane_refill_count(worlds, alphabet):
    """every lane searches 8 queries on average or more: counts, status bytes and the census of the device entry points on
    a batch that holds the four kinds of rejected query, and the host entry point on its accepted part"""
    t0 = time.time()
    w = worlds[alphabet]
    ix = w.ix
    lanes = resident_lanes()
    # device pool = pool + rejected queries (status != 0, all-zero rows)
    rq = [q for q, _ in REJECTED]
    db, do = pack_queries(w.q + rq)
    dcounts = np.concatenate([w.counts, np.zeros((len(rq), 3), np.uint64)])
    dstatus = np.concatenate([np.zeros(w.P, np.uint8), np.array([s for _, s in REJECTED], np.uint8)])
    n = 8 * lanes + lanes // 2
    p = np.concatenate([w.draw_weights(np.arange(w.P)) * 0.97, np.full(len(rq), 0.03 / len(rq))])
    draw = np.random.default_rng(101 + w.alphabet).choice(w.P + len(rq), size=n, p=p)
    accepted = dstatus[draw] == 0
    n_ok = int(accepted.sum())
    assert n_ok >= 8 * lanes and n - n_ok >= 1000 and all(int((draw == w.P + j).sum()) > 0 for j in range(len(rq)))
    assert 0 < float((w.len[draw[accepted]] > 64).mean()) <= 0.05
    o, b = gather(do, draw, db)
    d_q, d_o = ix.dev_upload(np.concatenate([b, np.zeros(16, np.uint8)])), ix.dev_upload(o)
    d_c, d_s, d_t = ix.dev_malloc(8 * n * 3), ix.dev_malloc(n), ix.dev_malloc(16)
    times = []
    try:
        for k in (0, 1, 2):
            for tally in (True, False):
                ix.dev_memset(d_c, 0xAB, 8 * n * 3)
                ix.dev_memset(d_s, 0xEE, n)
                ix.dev_memset(d_t, 0, 16)
                t1 = time.time()
                if tally:
                    ix.dev_count_mismatch_tally(d_q, d_o, n, k, d_c, d_t, d_s)
                else:
                    ix.dev_count_mismatch(d_q, d_o, n, k, d_c, d_s)
                ix.dev_synchronize()
                times.append(time.time() - t1)
                got = ix.dev_download(d_c, (n, k + 1), np.uint64)
                status = ix.dev_download(d_s, (n,), np.uint8)
                want = dcounts[draw][:, :k + 1]
                bad = np.flatnonzero((got != want).any(axis=1))
                assert len(bad) == 0, (k, tally, len(bad), bad[:5], got[bad[:5]], want[bad[:5]])
                assert np.array_equal(status, dstatus[draw]), (k, tally)
                assert not got[~accepted].any()
                if tally:
                    census = ix.dev_download(d_t, (2,), np.uint64)
                    assert int(census[1]) == n_ok, (k, census)  # (word 0 counts expansions: the reference has no value for it)
    finally:
        for ptr in (d_q, d_o, d_c, d_s, d_t):
            ix.dev_free(ptr)
    vdraw = draw[accepted]
    vb, vo = w.batch_bytes(vdraw)
    for k in (0, 1, 2):
        t1 = time.time()
        got = ix.parallel_count_mismatch_csr(vb, vo, k)
        times.append(time.time() - t1)
        assert np.array_equal(got, w.counts[vdraw][:, :k + 1]), k
    print("lane refill, count (alphabet %d): n = %d (%d accepted) >= 8 x %d lanes; device k = 0, 1, 2 with / without census %s s; "
          "host k = 0, 1, 2 %s s; test %.1f s" % (w.alphabet, n, n_ok, lanes, " ".join("%.2f" % t for t in times[:6]),
                                                   " ".join("%.2f" % t for t in times[6:]), time.time() - t0))


@both_alphabets
def test_lane_refill_locate(worlds, alphabet):
    """the EMIT pass with lanes that write the leaves of several queries one after the other: 4 x resident lanes draws of the
    located pool entries.  Entry i is drawn with weight min(1, 8 / hits_i), so a draw brings at most 8 hits per pool entry
    in expectation and the batch stays inside HIT_BUDGET (asserted on the drawn batch)."""
    t0 = time.time()
    w = worlds[alphabet]
    ix = w.ix
    lanes = resident_lanes()
    n = 4 * lanes
    ent = w.loc_ok
    p = w.draw_weights(ent) * np.minimum(1.0, 8.0 / np.maximum(1, w.tot[2][ent]))
    rows = np.random.default_rng(202 + w.alphabet).choice(len(ent), size=n, p=p / p.sum())
    draw = ent[rows]
    assert n >= 4 * lanes and int(w.tot[2][draw].sum()) <= HIT_BUDGET
    assert int((w.tot[2][draw] == 0).sum()) > n // 100 and int((w.tot[2][draw] > 8).sum()) > n // 100
    qb, qo = w.batch_bytes(draw)
    times = []
    try:
        for devices in ([0], [0, 0]):
            if len(devices) > 1:
                ix.set_devices(devices)
            for k in (1, 2):
                t1 = time.time()
                got = ix.parallel_locate_mismatch_csr(qb, qo, k)
                times.append(time.time() - t1)
                locate_equals(got, gather(w.loc[k][0], rows, *w.loc[k][1:]), (devices, k))
    finally:
        ix.set_devices([0])
    print("lane refill, locate (alphabet %d): n = %d = 4 x %d lanes, %d hits at k = 2; one replica k = 1, 2: %.2f %.2f s; two: %.2f %.2f s; "
          "test %.1f s" % ((w.alphabet, n, lanes, int(w.tot[2][draw].sum())) + tuple(times) + (time.time() - t0,)))


def test_sort_regimes(worlds, monkeypatch):
    """2^15 segments (every rocPRIM configuration of the segmented radix sort partitions from 3 000 on) whose leaf counts
    hold the four classes 0, 1..32, 33..512 and more than 512 -- each at least 1 % of the batch, the largest above 1 000 --
    taken from the reference's leaves per query.  Amino 3- and 4-mers at k = 2 are the large segments (on i.i.d. nucleotide
    text of this size no query has more than ~440 occurring variants: 10-mers, all 436 ACGT variants present).  The share of
    the large class is what half the hit budget allows, at most 10 %.  Then once more with the leaf capacity at 1/16 of the
    batch's leaves, which splits it four levels deep."""
    t0 = time.time()
    w = worlds[1]
    ix = w.ix
    n = 1 << 15
    lv = w.leaves[w.loc_ok]
    classes = [np.flatnonzero(lv == 0), np.flatnonzero((lv >= 1) & (lv <= 32)), np.flatnonzero((lv >= 33) & (lv <= 512)), np.flatnonzero(lv > 512)]
    assert all(len(c) >= 5 for c in classes), [len(c) for c in classes]
    heavy_mean = float(w.tot[2][w.loc_ok][classes[3]].mean())
    share3 = min(0.10, (HIT_BUDGET / 2) / (n * heavy_mean))
    shares = [0.35, 0.35, 0.30 - share3, share3]
    rng = np.random.default_rng(303)
    rows = np.concatenate([rng.choice(c, size=int(round(s * n))) for c, s in zip(classes, shares)])
    rows = np.concatenate([rows, rng.choice(classes[0], size=n - len(rows))])
    rows = rows[rng.permutation(n)]
    draw = w.loc_ok[rows]
    got_lv = w.leaves[draw]
    assert len(draw) >= 1 << 15
    for lo, hi in ((0, 0), (1, 32), (33, 512), (513, 1 << 62)):
        assert int(((got_lv >= lo) & (got_lv <= hi)).sum()) >= n // 100, (lo, hi)
    assert int(got_lv.max()) > 1000 and int(w.tot[2][draw].sum()) <= HIT_BUDGET
    qb, qo = w.batch_bytes(draw)
    want = gather(w.loc[2][0], rows, *w.loc[2][1:])
    t1 = time.time()
    locate_equals(ix.parallel_locate_mismatch_csr(qb, qo, 2), want, "default capacity")
    t2 = time.time()
    assert np.array_equal(ix.parallel_count_mismatch_csr(qb, qo, 2), w.counts[draw])
    monkeypatch.setenv("AWRY_MISMATCH_LEAF_CAP", str(int(got_lv.sum()) // 16))  # (read per call; restored when the test ends)
    t3 = time.time()
    locate_equals(ix.parallel_locate_mismatch_csr(qb, qo, 2), want, "capacity 1/16 of the leaves")
    t4 = time.time()
    print("sort regimes: %d segments, %d leaves (classes %s, largest %d), %d hits; locate %.2f s, with 1/16 capacity %.2f s; test %.1f s"
          % (n, int(got_lv.sum()), [int(((got_lv >= lo) & (got_lv <= hi)).sum()) for lo, hi in ((0, 0), (1, 32), (33, 512), (513, 1 << 62))],
             int(got_lv.max()), int(w.tot[2][draw].sum()), t2 - t1, t4 - t3, time.time() - t0))


def fixed_length_entries(w, L, classes):
    ent = np.flatnonzero((w.len == L) & np.isin(w.cls, classes))
    q2d = np.stack([np.frombuffer(w.q[i], np.uint8) for i in ent])
    return ent, q2d


def test_chunks_count_query_cut(worlds):
    """one awry_count_mismatch_batch call of 2^24 + 2^20 12-mers at k = 1: two chunks, the second written behind the first"""
    t0 = time.time()
    w = worlds[0]
    ent, q2d = fixed_length_entries(w, 12, ["sampled_12", "planted1_12", "planted2_12", "random_12"])
    assert len(ent) >= 100
    n = MAXQ + (1 << 20)
    rows = np.random.default_rng(404).integers(0, len(ent), size=n)
    qb, qo = synth.fixed_to_csr(q2d[rows])
    cuts = chunk_cuts(qo)
    assert cuts == [(0, MAXQ), (MAXQ, n)]  # (every row is a pool draw, the two next to the cut included)
    want = w.counts[ent[rows]][:, :2]
    assert len(np.unique(want[MAXQ - 64:MAXQ + 64], axis=0)) > 1 and int(want[MAXQ:].sum()) > 0
    t1 = time.time()
    got = w.ix.parallel_count_mismatch_csr(qb, qo, 1)
    t2 = time.time()
    bad = np.flatnonzero((got != want).any(axis=1))
    assert len(bad) == 0, (len(bad), bad[:5], got[bad[:5]], want[bad[:5]])
    print("chunks, query cut: %d queries, call %.2f s, test %.1f s" % (n, t2 - t1, time.time() - t0))


def test_chunks_count_byte_cut(worlds):
    """one call of 5.5 M 101-byte reads (more than 2^29 query bytes) at k = 0 and 1: the byte cut halves the batch"""
    t0 = time.time()
    w = worlds[0]
    ent, q2d = fixed_length_entries(w, 101, ["sampled_101", "planted1_101", "planted2_101", "random_101", "sampled_long", "planted1_long",
                                             "planted2_long", "random_long"])
    assert len(ent) >= 50
    n = 5_500_000
    rows = np.random.default_rng(505).integers(0, len(ent), size=n)
    qb, qo = synth.fixed_to_csr(q2d[rows])
    assert int(qo[-1]) > MAXB
    cuts = chunk_cuts(qo)
    assert cuts == [(0, n // 2), (n // 2, n)]
    times = []
    for k in (0, 1):
        want = w.counts[ent[rows]][:, :k + 1]
        assert int(want[:n // 2].sum()) > 0 and int(want[n // 2:].sum()) > 0
        t1 = time.time()
        got = w.ix.parallel_count_mismatch_csr(qb, qo, k)
        times.append(time.time() - t1)
        bad = np.flatnonzero((got != want).any(axis=1))
        assert len(bad) == 0, (k, len(bad), bad[:5], got[bad[:5]], want[bad[:5]])
    print("chunks, byte cut: %d reads, %d bytes, k = 0: %.2f s, k = 1: %.2f s, test %.1f s" % (n, int(qo[-1]), times[0], times[1], time.time() - t0))


def test_chunks_locate(worlds):
    """one awry_locate_mismatch_batch call of 2^24 + 2^18 20-mers at k = 1.  99 % are draws from 2^14 random 20-mers that the
    reference counts at zero for k = 1 (random 20-mers with a hit, about 1 in 4 000 on this text, are left out of that set), a
    seeded 1 % and the rows next to the cut are draws from the pool's 20-mers, most of which have hits: the concatenation over
    chunks has hits on both sides of the cut."""
    t0 = time.time()
    w = worlds[0]
    ent, q2d = fixed_length_entries(w, 20, ["sampled_20", "planted1_20", "planted2_20", "sampled", "planted1", "planted2"])
    assert len(ent) >= 250 and (w.loc_row[ent] >= 0).all()
    z2d = synth.random_queries(1 << 14, 20, 0, 606)
    zc, _ = mr.oracle_counts_batch(w.oi, [bytes(r) for r in z2d], 1, 0, THREADS)
    z2d = z2d[zc.sum(axis=1) == 0]
    Z = len(z2d)
    assert Z >= (1 << 14) - 64
    n = MAXQ + (1 << 18)
    rng = np.random.default_rng(707)
    rows = rng.integers(0, Z, size=n)
    hot = np.flatnonzero(rng.random(n) < 0.01)
    hot = np.unique(np.concatenate([hot, [MAXQ - 2, MAXQ - 1, MAXQ, MAXQ + 1]]))
    rows[hot] = Z + rng.integers(0, len(ent), size=len(hot))
    rows[[MAXQ - 1, MAXQ]] = Z + np.flatnonzero(w.tot[1][ent] > 0)[:2]     # a hit in the row on either side of the cut
    qb, qo = synth.fixed_to_csr(np.concatenate([z2d, q2d])[rows])
    assert chunk_cuts(qo) == [(0, MAXQ), (MAXQ, n)]
    off1, g1, p1, d1 = w.loc[1]
    lens = np.concatenate([np.zeros(Z, np.int64), np.diff(off1.astype(np.int64))[w.loc_row[ent]]])
    coff = np.zeros(len(lens) + 1, np.uint64)
    coff[1:] = np.cumsum(lens)
    _, cg, cp, cd = gather(off1, w.loc_row[ent], g1, p1, d1)
    want = gather(coff, rows, cg, cp, cd)
    assert int(want[0][MAXQ]) > 1000 and int(want[0][-1] - want[0][MAXQ]) > 100 and int(want[0][-1]) <= HIT_BUDGET
    t1 = time.time()
    got = w.ix.parallel_locate_mismatch_csr(qb, qo, 1)
    t2 = time.time()
    locate_equals(got, want, "two chunks")
    print("chunks, locate: %d queries, %d hits (%d behind the cut), call %.2f s, test %.1f s"
          % (n, int(want[0][-1]), int(want[0][-1] - want[0][MAXQ]), t2 - t1, time.time() - t0))


def test_wide_rows(worlds):
    """a replica on the 64-bit-row kernels (awry_debug_force_wide_rows; launch_locate over the leaf list takes the wide
    kernels): the pool in pool order through count and locate for k = 0, 1, 2 equals the reference and the narrow replica"""
    import awry_amd
    t0 = time.time()
    w = worlds[0]
    L_ = awry_amd.load_library()
    L_.awry_debug_force_wide_rows(1)
    try:
        wide = FmIndex.from_text(w.text, 0, 8, 0, w.st, w.hd).set_devices([0])
    finally:
        L_.awry_debug_force_wide_rows(0)
    try:
        assert "count_nt2_wide_kernel" in wide.count_schedule(31) and "count_nt2_wide_kernel" not in w.ix.count_schedule(31)
        lb, lo = gather(w.qo, w.loc_ok, w.qb)[::-1]
        for k in (0, 1, 2):
            c_wide, c_narrow = wide.parallel_count_mismatch_csr(w.qb, w.qo, k), w.ix.parallel_count_mismatch_csr(w.qb, w.qo, k)
            assert np.array_equal(c_wide, w.counts[:, :k + 1]) and np.array_equal(c_narrow, c_wide), k
            l_wide, l_narrow = wide.parallel_locate_mismatch_csr(lb, lo, k), w.ix.parallel_locate_mismatch_csr(lb, lo, k)
            locate_equals(l_wide, w.loc[k], ("wide", k))
            locate_equals(l_narrow, l_wide, ("narrow", k))
    finally:
        wide.close()
    print("wide rows: %d queries counted, %d located, %d hits at k = 2, test %.1f s" % (w.P, len(w.loc_ok), len(w.loc[2][1]), time.time() - t0))
