"""awry_count_schedule names the plan the launchers run (count_plan.h): on the repeat-rich 3 Mbp text, 101-bp reads with and
without the left-context index and 31-mers with and without the k-mer count table count what the oracle counts, and the report
names the lane-pass schedule / carries the table note exactly when the switch is on."""
import numpy as np
import pytest

from awry_amd.fm_index import FmIndex
from tests import synth

pytestmark = pytest.mark.gpu

READS_LANES = "count_nt2_reads_probe_kernel+lcx_quad_reads_kernel+count_nt2_reads_pool_kernel"
READS_LISTS = "count_nt2_reads_probe_kernel+count_nt2_reads_kernel"


@pytest.fixture(scope="module")
def world(oracle):
    text, st, hd, _ = synth.repeat_rich_text(3_000_000, seed=5, n_records=3, device="cpu", scale=2.0)
    ix = FmIndex.from_text(text, 0, 8, 0, st, hd).set_devices([0])
    oi = oracle.OracleIndex.from_text(text, 0, 8, 0, st, hd)
    reads = synth.sampled_queries(text, 5000, 101, 101)
    kmers = np.concatenate([synth.sampled_queries(text, 4000, 31, 31), synth.random_queries(1000, 31, 0, 32)])
    want = {101: oi.parallel_count(*synth.fixed_to_csr(reads), 8)[0], 31: oi.parallel_count(*synth.fixed_to_csr(kmers), 8)[0]}
    oi.close()
    assert ix.verify_enabled() and ix.locate_sa_ratio() == 1 and 1 <= ix.seed_kmer_len() <= 28
    return ix, reads, kmers, want


def dev_count_reads(ix, q2d):
    """dev_pack_nt2 -> dev_count_nt2_long on the NULL stream"""
    n, L = q2d.shape
    d_ascii = ix.dev_upload(np.ascontiguousarray(q2d).reshape(-1))
    d_words, d_counts, d_bad = ix.dev_malloc(8 * n * ((L + 31) // 32)), ix.dev_malloc(8 * n), ix.dev_malloc(8)
    try:
        ix.dev_memset(d_bad, 0, 8)
        ix.dev_pack_nt2(d_ascii, n, L, d_words, d_bad)
        ix.dev_count_nt2_long(d_words, n, L, d_counts)
        ix.dev_synchronize()
        assert int(ix.dev_download(d_bad, (1,), np.uint64)[0]) == 0
        return ix.dev_download(d_counts, (n,), np.uint64)
    finally:
        for p in (d_ascii, d_words, d_counts, d_bad):
            ix.dev_free(p)


def test_reads_with_and_without_the_lane_pass(world):
    ix, reads, _, want = world
    assert (want[101] > 1).sum() > 100, "the text should hold repeated reads"
    try:
        ix.set_lcx(True)
        assert ix.lcx_enabled() and ix.count_schedule(101) == READS_LANES
        assert np.array_equal(dev_count_reads(ix, reads), want[101])
        ix.set_lcx(False)
        assert not ix.lcx_enabled() and ix.count_schedule(101) == READS_LISTS
        assert np.array_equal(dev_count_reads(ix, reads), want[101])
    finally:
        ix.set_lcx(True)


def test_kmers_with_and_without_the_count_table(world):
    ix, _, kmers, want = world
    assert ix.lcx_enabled()
    try:
        ix.set_kmer_table(1)
        assert "k-mer count table" in ix.count_schedule(31) and ix.count_schedule(31).startswith("count_nt2_probe_resume_kernel (")
        assert np.array_equal(ix.count_kmers_nt2(kmers, True), want[31])
        assert ix.kmer_table_info()["length"] == 31
        ix.set_kmer_table(0)
        assert ix.count_schedule(31) == "count_nt2_probe_resume_kernel"
        assert np.array_equal(ix.count_kmers_nt2(kmers, True), want[31])
        assert ix.kmer_table_info()["length"] == 0
    finally:
        ix.set_kmer_table(-1)
