"""The work the packed count kernels do, not only what they return.  A start or step helper that takes one LF step too many
or probes the table twice still returns the right count; the census of awry_dev_count_nt2_tally (probes, steps, blocks ranked,
SA reads, text windows, deep blocks, left-context nodes, row positions) does not stay the same.  One small index with every
policy input set by hand, one batch of 4,099 k-mers per length (no multiple of 4, 64 or 256: a quad4 tail group, a partial
wave and a partial chunk), every single-kernel schedule with and without the seed table, the one-launch two-phase schedule,
and the wide-row kernels: counts are the oracle's, each census equals the constant below, and across schedules the probes are
n wherever a table is read and the steps of modes 0, 1 and 2 are one number.  reads_body keeps no census: ragged reads through
the host path pin its counts, range-start words and locations against the oracle, on both row widths.

The seed windows that are absent from the text exist for seed k = 8 only: a text of 200,000 letters holds all 1,024 5-mers."""
import numpy as np
import pytest

from awry_amd import _lib
from awry_amd.fm_index import FmIndex
from tests import synth

pytestmark = pytest.mark.gpu

N_QUERIES = 4099
SEED_KS = (5, 8)
LENGTHS = {5: (5, 6, 31, 32), 8: (8, 9, 31, 32)}  # k (i0 = 0), k + 1 (a singleton check with one letter left), shifts up to bit 62
# (debug mode, set_verify_kmers) of the single-kernel schedules: strided quads, chunks, groups of four, groups of four + verify
SINGLE = (("quad", 0, False), ("chunk", 1, False), ("quad4", 2, False), ("quad4v", 2, True))

# censuses of commit 50328f8 (the parent of the shared seed-entry start functions of kernels_quad.hip.h), keyed by (seed k or 0 for
# use_seed = False, L, schedule); "wide" / "wide3": the index under awry_debug_force_wide_rows(1), default schedule / mode 3
CENSUS = {}


def _parent(ks, L, schedules, probes, steps, blocks, sa=0, windows=0, deep=0):
    for name in schedules.split():
        CENSUS[(ks, L, name)] = (probes, steps, blocks, sa, windows, deep, 0, 0)  # (no position seeds at these k: no left-context index)


_parent(0, 5, "quad chunk quad4 quad4v", 0, 16396, 32792)
_parent(0, 6, "quad chunk quad4 quad4v", 0, 20495, 39969)
_parent(0, 8, "quad chunk quad4 quad4v", 0, 28693, 49161)
_parent(0, 9, "quad chunk quad4 quad4v", 0, 32683, 53248)
_parent(0, 31, "quad chunk", 0, 75073, 95783)
_parent(0, 31, "quad4", 0, 75073, 95783, deep=36573)
_parent(0, 31, "quad4v", 0, 28307, 48781, sa=16621, windows=16615)
_parent(0, 32, "quad chunk", 0, 77190, 97926)
_parent(0, 32, "quad4", 0, 77190, 97926, deep=38734)
_parent(0, 32, "quad4v", 0, 28261, 48723, sa=16856, windows=16851)
_parent(5, 5, "quad chunk quad4 quad4v twophase wide wide3", 4099, 0, 0)
_parent(5, 6, "quad chunk quad4 quad4v twophase wide wide3", 4099, 4099, 7177)
_parent(5, 31, "quad chunk wide wide3", 4099, 58677, 62991)
_parent(5, 31, "quad4", 4099, 58677, 62991, deep=27771)
_parent(5, 31, "quad4v twophase", 4099, 11911, 15989, sa=16621, windows=16615)
_parent(5, 32, "quad chunk wide wide3", 4099, 60794, 65134)
_parent(5, 32, "quad4", 4099, 60794, 65134, deep=29844)
_parent(5, 32, "quad4v twophase", 4099, 11865, 15931, sa=16856, windows=16851)
_parent(8, 8, "quad chunk quad4 quad4v twophase wide wide3", 4099, 0, 0)
_parent(8, 9, "quad chunk quad4 quad4v twophase wide wide3", 4099, 3703, 3763)
_parent(8, 31, "quad chunk wide wide3", 4099, 46212, 46435)
_parent(8, 31, "quad4", 4099, 46212, 46435, deep=21692)
_parent(8, 31, "quad4v twophase", 4099, 93, 96, sa=14077, windows=14072)
_parent(8, 32, "quad chunk wide wide3", 4099, 48309, 48575)
_parent(8, 32, "quad4", 4099, 48309, 48575, deep=23724)
_parent(8, 32, "quad4v twophase", 4099, 47, 48, sa=14266, windows=14264)


def census_run(ix, q2d, use_seed):
    q2d = np.ascontiguousarray(q2d, dtype=np.uint8)
    n, L = q2d.shape
    d_ascii = ix.dev_upload(q2d.reshape(-1))
    d_words, d_counts, d_bad, d_tally = ix.dev_malloc(8 * n), ix.dev_malloc(8 * n), ix.dev_malloc(8), ix.dev_malloc(64)
    try:
        ix.dev_memset(d_bad, 0, 8)
        ix.dev_memset(d_tally, 0, 64)
        ix.dev_pack_nt2(d_ascii, n, L, d_words, d_bad)
        ix.dev_count_nt2_tally(d_words, n, L, d_counts, d_tally, use_seed)
        ix.dev_synchronize()
        assert int(ix.dev_download(d_bad, (1,), np.uint64)[0]) == 0
        return ix.dev_download(d_counts, (n,), np.uint64), tuple(int(x) for x in ix.dev_download(d_tally, (8,), np.uint64))
    finally:
        for p in (d_ascii, d_words, d_counts, d_bad, d_tally):
            ix.dev_free(p)


def absent_windows(text, k):
    """one k-mer per last letter A, C, G, T that the text does not hold"""
    code = np.full(256, 4, dtype=np.int64)
    code[synth.NT] = np.arange(4)
    c = code[text]
    win = np.lib.stride_tricks.sliding_window_view(c, k)
    ok = (win < 4).all(axis=1)
    keys = (win[ok] * (4 ** np.arange(k - 1, -1, -1))).sum(axis=1)
    seen = np.zeros(4 ** k, dtype=bool)
    seen[keys] = True
    out = []
    for last in range(4):
        cand = np.flatnonzero(~seen)
        cand = cand[cand % 4 == last]
        assert len(cand), "no absent %d-mer ends in %s" % (k, "ACGT"[last])
        v = int(cand[len(cand) // 2])
        out.append(synth.NT[[(v >> (2 * (k - 1 - j))) & 3 for j in range(k)]])
    return np.stack(out)


def kmer_batch(text, L, absent8):
    """a third from the text, a third from the text with one substitution, a third random, and four that end in absent windows"""
    rng = np.random.default_rng(1000 + L)
    pres = synth.sampled_queries(text, 1367, L, 50 + L)
    near = synth.sampled_queries(text, 1366, L, 90 + L)
    col = rng.integers(0, L, size=len(near))
    near[np.arange(len(near)), col] = synth.NT[(np.searchsorted(synth.NT, near[np.arange(len(near)), col]) + 1) % 4]
    rand = synth.random_queries(1362, L, 0, 130 + L)
    tail = synth.random_queries(4, L, 0, 170 + L)
    m = min(L, absent8.shape[1])
    tail[:, L - m:] = absent8[:, absent8.shape[1] - m:]
    q2d = np.concatenate([pres, near, rand, tail])
    q2d = q2d[rng.permutation(len(q2d))]
    assert q2d.shape == (N_QUERIES, L)
    return q2d


@pytest.fixture(scope="module")
def world(oracle):
    text, st, hd = synth.make_text(200_000, 0, 20261, 2, 0.01)
    assert len(st) == 2 and (text == ord("N")).sum() > 100
    oi = oracle.OracleIndex.from_text(text, 0, 8, 0, st, hd)
    L_ = _lib.load_library()
    narrow = FmIndex.from_text(text, 0, 8, 0, st, hd).set_devices([0])
    narrow.set_locate_sa_ratio(1)
    narrow.set_verify(0)
    narrow.set_lcx(True)
    L_.awry_debug_force_wide_rows(1)
    try:
        wide = FmIndex.from_text(text, 0, 8, 0, st, hd).set_devices([0])
    finally:
        L_.awry_debug_force_wide_rows(0)
    # The wide index has one policy input, the seed k (set per test).  The others cannot be set on it: the dense SA, the verify
    # accelerators and the left-context index are 32-bit structures, and awry_set_locate_sa_ratio / awry_set_verify refuse wide rows (error -6), so
    # nothing there can depend on free memory; the schedule of the wide kernels follows the debug mode alone.
    assert narrow.verify_enabled() and not wide.verify_enabled()
    assert "count_nt2_wide_kernel" in wide.count_schedule(31) and "count_nt2_wide_kernel" not in narrow.count_schedule(31)
    absent8 = absent_windows(text, 8)
    batches = {}
    for L in sorted({L for k in SEED_KS for L in LENGTHS[k]}):
        q2d = kmer_batch(text, L, absent8)
        batches[L] = (q2d, oi.parallel_count(*synth.fixed_to_csr(q2d), 4)[0])
    absent_counts = oi.parallel_count(*synth.fixed_to_csr(absent8), 4)[0]
    assert not absent_counts.any() and bytes(absent8[:, -1]) == b"ACGT"
    return dict(text=text, oi=oi, L_=L_, narrow=narrow, wide=wide, batches=batches)


def measured_censuses(world, k):
    """{(k or 0, L, schedule): census} of every schedule at seed k, counts checked against the oracle on the way"""
    L_, narrow, wide = world["L_"], world["narrow"], world["wide"]
    out = {}
    narrow.set_seed_kmer_len(k)
    wide.set_seed_kmer_len(k)
    assert narrow.seed_kmer_len() == k and wide.seed_kmer_len() == k
    try:
        for L in LENGTHS[k]:
            q2d, want = world["batches"][L]
            for name, mode, vk in SINGLE:
                L_.awry_debug_set_count_kernel(mode)
                narrow.set_verify_kmers(vk)
                for use_seed in (True, False):
                    got, census = census_run(narrow, q2d, use_seed)
                    assert np.array_equal(got, want), (k, L, name, use_seed)
                    assert np.array_equal(narrow.count_kmers_nt2(q2d, use_seed), want), (k, L, name, use_seed)  # the production instantiation
                    out[(k if use_seed else 0, L, name)] = census  # (key 0: the same constants are asked of both seed k)
            narrow.set_verify_kmers(False)
            L_.awry_debug_set_count_kernel(3)
            assert narrow.count_schedule(L) == "count_nt2_probe_resume_kernel"
            for ix, name in ((narrow, "twophase"), (wide, "wide3")):
                got, out[(k, L, name)] = census_run(ix, q2d, True)
                assert np.array_equal(got, want), (k, L, name)
                assert np.array_equal(ix.count_kmers_nt2(q2d, True), want), (k, L, name)
            L_.awry_debug_set_count_kernel(-1)
            got, out[(k, L, "wide")] = census_run(wide, q2d, True)
            assert np.array_equal(got, want), (k, L, "wide")
            assert np.array_equal(wide.count_kmers_nt2(q2d, True), want), (k, L, "wide")
    finally:
        L_.awry_debug_set_count_kernel(-1)
        narrow.set_verify_kmers(False)
    return out


@pytest.mark.parametrize("k", SEED_KS)
def test_census_of_every_schedule(world, k):
    got = measured_censuses(world, k)
    n = N_QUERIES
    for L in LENGTHS[k]:
        for name in ("quad", "chunk", "quad4", "quad4v", "twophase", "wide", "wide3"):
            assert got[(k, L, name)][0] == n, (k, L, name)  # one probe per query wherever a table is read
        for ks in (k, 0):
            steps = {got[(ks, L, name)][1] for name in ("quad", "chunk", "quad4")}
            assert len(steps) == 1, (ks, L, steps)  # the same searches, whichever schedule hands them out
        for name, _, _ in SINGLE:
            assert got[(0, L, name)][0] == 0, (L, name)  # no table, no probe
        assert got[(0, L, "quad")][1] <= n * (L - 1)
        assert got[(k, L, "wide")][1:3] == got[(k, L, "quad")][1:3], (k, L)  # 64-bit rows: the same steps and blocks
        if L == k:
            assert got[(k, L, "quad")][1] == 0  # the entry is the answer
    want = {key: c for key, c in CENSUS.items() if key[0] == k or (key[0] == 0 and key[1] in LENGTHS[k])}
    assert got == want


def ragged_reads(text, k):
    """611 reads: most of 20..150 letters, and some shorter than the seed k or with fewer than 3 letters left of its window"""
    rng = np.random.default_rng(611)
    nq = 611
    lens = rng.integers(20, 151, size=nq)
    short = rng.choice(nq, size=48, replace=False)
    lens[short] = np.resize(np.arange(1, k + 3), len(short))
    starts = rng.integers(0, len(text) - 160, size=nq)
    qs = []
    for i in range(nq):
        q = text[starts[i]:starts[i] + lens[i]].copy()
        if i % 3 == 1:  # not from the text
            q = synth.NT[rng.integers(0, 4, size=lens[i])]
        elif i % 3 == 2:  # from the text, one substitution
            j = int(rng.integers(0, lens[i]))
            q[j] = synth.NT[(int(np.searchsorted(synth.NT, q[j])) + 1) % 4] if q[j] in synth.NT else ord("A")
        if not np.isin(q, synth.NT).all():
            q = synth.NT[rng.integers(0, 4, size=lens[i])]
        qs.append(q)
    qo = np.zeros(nq + 1, dtype=np.uint64)
    qo[1:] = np.cumsum(lens)
    return np.concatenate(qs), qo, lens


def test_ragged_reads_on_both_schedules_and_row_widths(world):
    L_, oi = world["L_"], world["oi"]
    k = 8
    qb, qo, lens = ragged_reads(world["text"], k)
    assert (lens < k).sum() >= 8 and ((lens >= k) & (lens - k < 3)).sum() >= 8 and lens.max() > 128
    want = oi.parallel_locate(qb, qo, 4)[:3]
    assert 100 < (np.diff(want[0]) > 0).sum() < len(lens)
    try:
        for name in ("narrow", "wide"):
            ix = world[name]
            ix.set_seed_kmer_len(k)
            # narrow rows: the two-phase schedule, the single kernel, the two-phase schedule by request; wide rows: -1 and 0 are
            # the one single kernel, 3 the probe pass + listed quads with per-read lengths
            for mode in (-1, 0, 3):
                L_.awry_debug_set_count_kernel(mode)
                got = ix.parallel_locate_csr(qb, qo)
                for x, y, what in zip(got, want, ("offsets", "global positions", "record positions")):
                    assert np.array_equal(x, y), (name, mode, what)
                assert np.array_equal(ix.parallel_count_csr(qb, qo), np.diff(want[0])), (name, mode)
    finally:
        L_.awry_debug_set_count_kernel(-1)
