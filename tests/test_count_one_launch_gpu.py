"""The two-phase k-mer schedule as one launch (count_nt2_probe_resume_kernel, debug mode 3) against the same phases as two
launches (count_nt2_probe_kernel + count_nt2_resume_kernel, debug modes 4 and 5): identical counts, identical work census, and
both the oracle's -- on random batches and on k-mers of a repeat-rich text (many left-context survivors), for L = k, L < k
(a rung table), L = 31 and 32, and batch sizes from one query to more than the grid holds in one pass."""
import numpy as np
import pytest

from awry_amd import _lib
from awry_amd.fm_index import FmIndex
from tests import synth

pytestmark = pytest.mark.gpu


def count_with_census(ix, q2d):
    """counts and the whole 8-word census of awry_dev_count_nt2_tally (probes, steps, blocks, SA reads, text windows, deep
    blocks, left-context nodes, row positions)"""
    q2d = np.ascontiguousarray(q2d, dtype=np.uint8)
    n, L = q2d.shape
    d_ascii = ix.dev_upload(q2d.reshape(-1))
    d_words, d_counts, d_bad, d_tally = ix.dev_malloc(8 * n), ix.dev_malloc(8 * n), ix.dev_malloc(8), ix.dev_malloc(64)
    try:
        ix.dev_memset(d_bad, 0, 8)
        ix.dev_memset(d_tally, 0, 64)
        ix.dev_pack_nt2(d_ascii, n, L, d_words, d_bad)
        ix.dev_count_nt2_tally(d_words, n, L, d_counts, d_tally, True)
        ix.dev_synchronize()
        assert int(ix.dev_download(d_bad, (1,), np.uint64)[0]) == 0
        return ix.dev_download(d_counts, (n,), np.uint64), ix.dev_download(d_tally, (8,), np.uint64)
    finally:
        for p in (d_ascii, d_words, d_counts, d_bad, d_tally):
            ix.dev_free(p)


@pytest.fixture(scope="module")
def repeat_index():
    text, st, hd, _ = synth.repeat_rich_text(3_000_000, seed=5, n_records=3, device="cpu", scale=2.0)
    return text, st, hd, FmIndex.from_text(text, 0, 8, 0, st, hd).set_devices([0])


def test_one_launch_equals_the_pair_and_the_oracle(oracle, repeat_index):
    text, st, hd, ix = repeat_index
    oi = oracle.OracleIndex.from_text(text, 0, 8, 0, st, hd)
    L_ = _lib.load_library()
    k = ix.seed_kmer_len()
    rng = np.random.default_rng(3)
    lcx_nodes = 0
    try:
        for L in (31, 32, k):
            pres = synth.sampled_queries(text, 40_000, L, L)
            near = pres[:10_000].copy()  # one substitution: survivors of the probe that the text or the keys decide
            col = rng.integers(0, L, size=len(near))
            near[np.arange(len(near)), col] = synth.NT[(np.searchsorted(synth.NT[:4], near[np.arange(len(near)), col]) + 1) % 4]
            rand = synth.random_queries(450_000, L, 0, L + 7)  # with the rest: more queries than the grid takes in one pass
            q2d = np.concatenate([pres, near, rand])
            q2d = q2d[rng.permutation(len(q2d))]
            want, _ = oi.parallel_count(*synth.fixed_to_csr(q2d), 8)
            assert (want > 100).sum() > 10, "the text should hold high-copy k-mers"
            for nq in (1, 63, 64, 1025, 5000, len(q2d)):
                censuses = []
                for mode, name in ((3, "count_nt2_probe_resume_kernel"), (4, "count_nt2_probe_kernel+count_nt2_resume_kernel"),
                                   (5, "count_nt2_probe_kernel+count_nt2_resume_kernel")):
                    L_.awry_debug_set_count_kernel(mode)
                    assert ix.count_schedule(L) == name
                    # the production instantiation (no census) and the census one: each on the grid it launches with
                    assert np.array_equal(ix.count_kmers_nt2(q2d[:nq], True), want[:nq]), (L, nq, mode)
                    got, census = count_with_census(ix, q2d[:nq])
                    assert np.array_equal(got, want[:nq]), (L, nq, mode)
                    censuses.append(census)
                c1 = censuses[0]
                for c in censuses[1:]:
                    assert np.array_equal(c1, c), (L, nq, c1, c)
                assert int(c1[0]) == nq
            lcx_nodes += int(c1[6])
    finally:
        L_.awry_debug_set_count_kernel(-1)
    if ix.lcx_enabled():
        assert lcx_nodes > 0, "the left-context index should have decided survivors of the probe"


def test_rung_table_takes_the_one_launch(oracle, repeat_index):
    """L < k: the rung table's entries are the answer; the schedule is the one launch"""
    text, st, hd, ix = repeat_index
    oi = oracle.OracleIndex.from_text(text, 0, 8, 0, st, hd)
    L = ix.seed_kmer_len() - 2
    q2d = np.concatenate([synth.sampled_queries(text, 6000, L, 41), synth.random_queries(6000, L, 0, 42)])
    want, _ = oi.parallel_count(*synth.fixed_to_csr(q2d), 8)
    assert "count_nt2_probe_resume_kernel" in ix.count_schedule(L) and "table of its own" in ix.count_schedule(L)
    for nq in (len(q2d), 4096):
        got, census = count_with_census(ix, q2d[:nq])
        assert np.array_equal(got, want[:nq]), nq
        assert int(census[0]) == nq
