"""GPU tests of the k-mer count table (awry_amd/csrc/kmer_table.hip.h, layout.h KT_*): for one k-mer length at a time, every
distinct L-mer of the seed buckets phase 2 of the k-mer count would search, with its count, in a hash table of 128-B lines.
Counts are the oracle's with the table on, off, far too small, rebuilt for another length and dropped; results never depend
on it.

How "the table settled a query" is measured.  Census word 6 counts index lines: one per table line read, one per line of a
search.  A batch made only of k-mers whose seed bucket has more than 4 rows (T of them, known from the oracle) sends every
query to the table, so its census is T + (lines of the searches of the queries the table did not settle), and a search is
at least one line: at least 2 T - census[6] queries were settled by their table line alone."""
import threading

import numpy as np
import pytest

from awry_amd.fm_index import FmIndex
from tests import synth
from tests.test_lcx_gpu import FAMILIES, family_text

pytestmark = pytest.mark.gpu

N_TEXT, SEED = 1_500_000, 3
LANE_ROWS = 4  # LCX_LANE_ROWS: buckets of up to this many rows are settled by a lane of the probe pass


def census_run(ix, q2d, stream=None):
    """counts and the 8-word census of awry_dev_count_nt2_tally"""
    q2d = np.ascontiguousarray(q2d, dtype=np.uint8)
    n, L = q2d.shape
    d_ascii = ix.dev_upload(q2d.reshape(-1))
    d_words, d_counts, d_bad, d_tally = ix.dev_malloc(8 * n), ix.dev_malloc(8 * n), ix.dev_malloc(8), ix.dev_malloc(64)
    try:
        ix.dev_memset(d_bad, 0, 8)
        ix.dev_memset(d_tally, 0, 64)
        ix.dev_pack_nt2(d_ascii, n, L, d_words, d_bad)
        ix.dev_synchronize()
        assert int(ix.dev_download(d_bad, (1,), np.uint64)[0]) == 0
        ix.dev_count_nt2_tally(d_words, n, L, d_counts, d_tally, True)
        ix.dev_synchronize()
        return ix.dev_download(d_counts, (n,), np.uint64), ix.dev_download(d_tally, (8,), np.uint64)
    finally:
        for p in (d_ascii, d_words, d_counts, d_bad, d_tally):
            ix.dev_free(p)


def substituted(q2d, rng):
    near = q2d.copy()
    col = rng.integers(0, q2d.shape[1], size=len(near))
    near[np.arange(len(near)), col] = synth.NT[(np.searchsorted(synth.NT[:4], near[np.arange(len(near)), col]) + 1) % 4]
    return near


class World:
    """the text of tests/test_lcx_gpu.py, its index and oracle, and per length the batch with its expected counts (computed once)"""

    def __init__(self, oracle):
        self.text, st, hd = family_text(N_TEXT, SEED, [(u, c * N_TEXT // 3_000_000, d) for u, c, d in FAMILIES], 3, 0.02)
        self.ix = FmIndex.from_text(self.text, 0, 8, 0, st, hd).set_devices([0])
        self.oi = oracle.OracleIndex.from_text(self.text, 0, 8, 0, st, hd)
        assert self.ix.lcx_enabled() and self.ix.verify_enabled()
        assert self.ix.kmer_table_info()["length"] == 0, "placing the index on a device builds no table"
        self.k = self.ix.seed_kmer_len()
        self.cache = {}

    def batch(self, L):
        """-> (q2d, expected counts, the present k-mers whose seed bucket has more than LANE_ROWS rows, number of present k-mers)"""
        if L not in self.cache:
            rng = np.random.default_rng(100 + L)
            pres = synth.sampled_queries(self.text, 6000, L, SEED + L)
            q2d = np.concatenate([pres, substituted(pres[:3000], rng), synth.random_queries(1500, L, 0, L)])
            want, _ = self.oi.parallel_count(*synth.fixed_to_csr(q2d), 4)
            rows, _ = self.oi.parallel_count(*synth.fixed_to_csr(np.ascontiguousarray(pres[:, L - self.k:])), 4)
            self.cache[L] = (q2d, want, np.ascontiguousarray(pres[rows > LANE_ROWS]), len(pres))
        return self.cache[L]

    def settled(self, L):
        """a lower bound on the present k-mers of batch(L) that the resident table settled from one line (module docstring)"""
        _, _, cov, _ = self.batch(L)
        info = self.ix.kmer_table_info()
        assert info["length"] == L and info["entries"] > 0 and info["lines"] * 128 == info["bytes"], info
        got, census = census_run(self.ix, cov)
        want, _ = self.oi.parallel_count(*synth.fixed_to_csr(cov), 4)
        assert np.array_equal(got, want)
        print("L = %d: %d covered k-mers, census[6] = %d, table %r" % (L, len(cov), int(census[6]), info))
        return 2 * len(cov) - int(census[6])

    def assert_table_used(self, L):
        _, _, _, n_pres = self.batch(L)
        s = self.settled(L)
        assert s >= 0.30 * n_pres, ("the table should settle at least 30 % of the present k-mers", L, s, n_pres)

    def close(self):
        self.ix.close()
        self.oi.close()


@pytest.fixture(scope="module")
def world(oracle):
    w = World(oracle)
    yield w
    w.ix.set_kmer_table(-1)
    w.close()


def check_counts(w, L, with_host_path=True):
    q2d, want, _, _ = w.batch(L)
    got, census = census_run(w.ix, q2d)
    assert np.array_equal(got, want), L
    assert np.array_equal(w.ix.count_kmers_nt2(q2d, True), want), L  # the production instantiation
    if with_host_path:
        assert np.array_equal(w.ix.parallel_count_csr(*synth.fixed_to_csr(q2d)), want), L
    return census


@pytest.mark.parametrize("L", [31, 21, 32, "k+1"])
def test_counts_match_the_oracle_with_the_table_on_and_off(world, L):
    w = world
    L = w.k + 1 if L == "k+1" else L
    w.ix.set_kmer_table(1)
    assert "k-mer count table" in w.ix.count_schedule(L) and "count_nt2_probe_resume_kernel" in w.ix.count_schedule(L)
    census_on = check_counts(w, L)
    w.assert_table_used(L)
    assert int(census_on[1]) <= len(w.batch(L)[0]) // 50, ("LF steps should be the exception", census_on)
    w.ix.set_kmer_table(0)
    assert w.ix.kmer_table_info()["length"] == 0
    census_off = check_counts(w, L)
    assert int(census_on[6]) < int(census_off[6]), ("one table line should replace the lines of a search", census_on, census_off)
    assert int(census_on[0]) == int(census_off[0]) == len(w.batch(L)[0])  # one seed probe per query either way


@pytest.mark.parametrize("L", [31, 21])
def test_a_table_far_too_small_overflows_and_counts_stay_right(world, L):
    """the same batch with the table forced to 64 lines: nearly every key finds its line full (L = 31: or its tag too wide for
    so few line bits), the getter reports the overflowed lines, and every such query is searched as without the table.  (That
    the table of the policy's size carries this batch is asserted first: here the table must NOT settle it.)"""
    from awry_amd import _lib
    w = world
    w.ix.set_kmer_table(0)
    w.ix.set_kmer_table(1)
    check_counts(w, L, False)
    w.assert_table_used(L)
    w.ix.set_kmer_table(0)
    _lib.load_library().awry_debug_set_kmer_table_lines(64)
    try:
        w.ix.set_kmer_table(1)
        check_counts(w, L)
        info = w.ix.kmer_table_info()
        assert info["length"] == L and info["lines"] == 64, info
        assert info["overflowed_lines"] > 32, ("most lines should have overflowed", info)
        assert info["entries"] <= 64 * 16, info
    finally:
        _lib.load_library().awry_debug_set_kmer_table_lines(0)
        w.ix.set_kmer_table(0)


def test_incomplete_left_contexts(oracle):
    """200 exact copies of a 60-letter unit in an i.i.d. text; in half of them an N sits 21..32 letters in front of the window
    the k-mers end in -- the 32-letter key of such a row is incomplete, its L - k nearest letters are not -- and one copy sits at
    the very start of the text.  The builder reads those letters from the text: the k-mers drawn across the copies count as
    the oracle says, settled by the table, and identically without it."""
    n, L, unit_len, copies = 300_000, 31, 60, 200
    rng = np.random.default_rng(17)
    body = synth.NT[rng.integers(0, 4, size=n, dtype=np.uint8)]
    unit = synth.NT[rng.integers(0, 4, size=unit_len, dtype=np.uint8)]
    slot = n // copies
    starts = [0] + [j * slot + int(rng.integers(100, slot - unit_len - 100)) for j in range(1, copies)]
    for s in starts:
        body[s:s + unit_len] = unit
    text = np.concatenate([body, np.frombuffer(b"$", np.uint8)])
    ix0 = FmIndex.from_text(text, 0, 8, 0, [0], ["seq0"]).set_devices([0])
    k = ix0.seed_kmer_len()
    ix0.close()
    assert 8 <= k < L and unit_len - k - 32 >= 0
    # the k-mers end in the unit's last k letters; the N of copy j (odd j) sits d_j letters in front of that window, L - k < d_j <= 32
    for j, s in enumerate(starts):
        if j % 2 == 1:
            d = L - k + 1 + (j // 2) % (32 - (L - k))
            assert L - k < d <= 32
            body[s + unit_len - k - d] = ord("N")
    text = np.concatenate([body, np.frombuffer(b"$", np.uint8)])
    ix = FmIndex.from_text(text, 0, 8, 0, [0], ["seq0"]).set_devices([0])
    oi = oracle.OracleIndex.from_text(text, 0, 8, 0, [0], ["seq0"])
    try:
        assert ix.lcx_enabled() and ix.seed_kmer_len() == k
        qs = []
        for s in starts[:40]:  # every window of the copy that ends inside the unit, the first copy's (at the text's start) included
            for e in range(L, unit_len + 1):
                q = text[s + e - L:s + e]
                if ord("N") not in q:
                    qs.append(q)
        pres = np.array(qs, dtype=np.uint8)
        q2d = np.concatenate([pres, substituted(pres[::3], rng), synth.random_queries(300, L, 0, 5)])
        want, _ = oi.parallel_count(*synth.fixed_to_csr(q2d), 4)
        ending = np.array([text[s + unit_len - L:s + unit_len] for s in starts[2:4]], dtype=np.uint8)  # (copy 3 has its N in front of the L-mer)
        assert (oi.parallel_count(*synth.fixed_to_csr(ending), 4)[0] == copies).all(), "the incomplete rows count for the k-mers that end the unit"
        rows, _ = oi.parallel_count(*synth.fixed_to_csr(np.ascontiguousarray(pres[:, L - k:])), 4)
        cov = np.ascontiguousarray(pres[rows > LANE_ROWS])
        assert len(cov) >= 0.9 * len(pres)
        ix.set_kmer_table(1)
        got, _ = census_run(ix, q2d)
        assert np.array_equal(got, want)
        info = ix.kmer_table_info()
        assert info["length"] == L and info["entries"] > 0, info
        got_cov, census = census_run(ix, cov)
        assert np.array_equal(got_cov, oi.parallel_count(*synth.fixed_to_csr(cov), 4)[0])
        print("incomplete contexts: %d covered k-mers, census[6] = %d, table %r" % (len(cov), int(census[6]), info))
        assert 2 * len(cov) - int(census[6]) >= 0.30 * len(pres), (len(cov), census, info)
        assert np.array_equal(ix.parallel_count_csr(*synth.fixed_to_csr(q2d)), want)
        ix.set_kmer_table(0)
        got, _ = census_run(ix, q2d)
        assert np.array_equal(got, want)
    finally:
        ix.close()
        oi.close()


def test_a_change_of_length_replaces_the_table(world):
    w = world
    w.ix.set_kmer_table(0)
    w.ix.set_kmer_table(1)
    for L in (31, 21, 31):
        check_counts(w, L, False)
        assert w.ix.kmer_table_info()["length"] == L
        w.assert_table_used(L)
    w.ix.set_kmer_table(0)


def test_what_drops_the_index_drops_the_table(world):
    w, L = world, 31
    q2d, want, _, _ = w.batch(L)
    w.ix.set_kmer_table(0)
    w.ix.set_kmer_table(1)
    check_counts(w, L, False)
    assert w.ix.kmer_table_info()["length"] == L
    try:
        w.ix.set_lcx(False)
        assert w.ix.kmer_table_info()["length"] == 0
        got, census = census_run(w.ix, q2d)
        assert np.array_equal(got, want) and int(census[6]) == 0, census
        assert w.ix.kmer_table_info()["length"] == 0
        w.ix.set_lcx(True)
        check_counts(w, L, False)
        assert w.ix.kmer_table_info()["length"] == L
        w.ix.set_verify(-1)
        assert w.ix.kmer_table_info()["length"] == 0
        got, census = census_run(w.ix, q2d)
        assert np.array_equal(got, want) and int(census[6]) == 0, census
        assert w.ix.kmer_table_info()["length"] == 0
    finally:
        w.ix.set_verify(2)
        w.ix.set_lcx(True)
    assert w.ix.lcx_enabled() and w.ix.verify_enabled()
    w.ix.set_kmer_table(1)
    check_counts(w, L, False)
    w.assert_table_used(L)
    w.ix.set_kmer_table(0)


def test_policy_builds_for_large_batches_only(world):
    w, L = world, 31
    q2d, want, _, _ = w.batch(L)
    w.ix.set_kmer_table(0)
    _, census_parent = census_run(w.ix, q2d[:4099])  # (mode 0: the searches of the parent)
    w.ix.set_kmer_table(-1)
    assert "k-mer count table" in w.ix.count_schedule(L)
    got, census = census_run(w.ix, q2d[:4099])
    assert np.array_equal(got, want[:4099])
    assert w.ix.kmer_table_info()["length"] == 0, "a batch of 4099 k-mers builds no table"
    assert np.array_equal(census, census_parent), (census, census_parent)
    big = np.concatenate([q2d] * 7)[:65536]
    assert len(big) == 65536
    got, _ = census_run(w.ix, big)
    assert np.array_equal(got, np.concatenate([want] * 7)[:65536])
    info = w.ix.kmer_table_info()
    assert info["length"] == L and info["entries"] > 0, info
    got, census = census_run(w.ix, q2d[:4099])  # a small batch keeps the searches of the parent, table or not
    assert np.array_equal(got, want[:4099]) and np.array_equal(census, census_parent)
    w.ix.set_kmer_table(0)


def test_first_use_from_two_host_threads_on_two_streams(world):
    import torch
    w, L = world, 21
    q2d, want, _, _ = w.batch(L)
    n = len(q2d)
    w.ix.set_kmer_table(0)
    w.ix.set_kmer_table(1)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    d_ascii = w.ix.dev_upload(np.ascontiguousarray(q2d).reshape(-1))
    d_words, d_bad = w.ix.dev_malloc(8 * n), w.ix.dev_malloc(8)
    d_counts = [w.ix.dev_malloc(8 * n), w.ix.dev_malloc(8 * n)]
    errors, gate = [], threading.Barrier(2)
    try:
        w.ix.dev_memset(d_bad, 0, 8)
        w.ix.dev_pack_nt2(d_ascii, n, L, d_words, d_bad)
        for d in d_counts:
            w.ix.dev_memset(d, 0xFF, 8 * n)
        w.ix.dev_synchronize()

        def run(i):
            try:
                torch.cuda.set_device(0)
                gate.wait()
                w.ix.dev_count_nt2(d_words, n, L, d_counts[i], True, streams[i].cuda_stream)
                streams[i].synchronize()
            except BaseException as e:  # noqa: BLE001
                errors.append(repr(e))

        threads = [threading.Thread(target=run, args=(i,)) for i in range(2)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        assert not errors, errors
        for d in d_counts:
            assert np.array_equal(w.ix.dev_download(d, (n,), np.uint64), want)
        info = w.ix.kmer_table_info()
        assert info["length"] == L and info["entries"] > 0, info
        w.assert_table_used(L)
        assert w.ix.kmer_table_info() == info, "one table: the second thread found the first one's"
    finally:
        for p in [d_ascii, d_words, d_bad] + d_counts:
            w.ix.dev_free(p)
        w.ix.set_kmer_table(0)
