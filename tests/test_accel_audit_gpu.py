"""Whole-structure audits of the device-only accelerators against a host recomputation from the text (tests/accel_ref.py, itself
checked against the definition in tests/test_accel_ref_cpu.py): the seed table in every encoding -- rows, position seeds with
14 + E context letters, the left-context index's flags, 16-byte wide entries, the amino contexts and symbol masks, the rungs --
the dense SA, the text as 4-bit and 8-bit codes, the SA of the N block and the sampled levels of the left-context index.
Nothing has a tolerance: the text determines every word, and every comparison is over the whole structure."""
import contextlib

import numpy as np
import pytest

import awry_amd
from awry_amd.fm_index import FmIndex
from tests import accel_ref as ar
from tests import synth
from tests.test_lcx_gpu import family_text

pytestmark = pytest.mark.gpu

L_ = awry_amd.load_library()
TEXTS = {
    "5k": lambda: synth.make_text(5_400, 0, 3, 3, 0.02),
    "20k": lambda: synth.make_text(20_000, 0, 61, 2, 0.02),
    "90k": lambda: synth.make_text(90_000, 0, 5, 3, 0.03),
    "family": lambda: family_text(600_000, 5, [(300, 1500, 0.10), (120, 4000, 0.03), (2000, 40, 0.02)], 3, 0.02),
    "amino": lambda: synth.make_text(20_000, 1, 62, 3, 0.01),
}
DEFAULT_K_E = {"5k": (8, 9), "20k": (9, 8), "90k": (11, 7), "family": (12, 6), "amino": (4, 0)}  # the seed policy's k, and E of the text's size
_worlds = {}


def world(name):
    """(text, record starts, headers, host reference): computed once per text for the module"""
    if name not in _worlds:
        text, st, hd = TEXTS[name]()
        _worlds[name] = (text, st, hd, ar.AccelRef(text, st, 1 if name == "amino" else 0))
    return _worlds[name]


def teardown_module(module):
    _worlds.clear()
    assert L_.awry_debug_max_blocks() == 0


@contextlib.contextmanager
def max_blocks(b):
    assert L_.awry_debug_set_max_blocks(b) == 0
    try:
        yield
    finally:
        L_.awry_debug_set_max_blocks(0)


@contextlib.contextmanager
def ctx_extra_cap(cap):
    assert L_.awry_debug_set_ctx_extra_cap(cap) == 0
    try:
        yield
    finally:
        L_.awry_debug_set_ctx_extra_cap(-1)


@contextlib.contextmanager
def wide_rows():
    L_.awry_debug_force_wide_rows(1)
    try:
        yield
    finally:
        L_.awry_debug_force_wide_rows(0)


def same(got, want, what, per_word=1):
    if np.array_equal(got, want):
        return
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero(got != want)
    i = int(bad[0])
    raise AssertionError("%s: %d of %d words differ, the first at %d (text position / row %d): got 0x%x, want 0x%x"
                         % (what, len(bad), len(want), i, i * per_word, int(got[i]), int(want[i])))


def audit(ix, ref, what, k, seed_pos, extra, lcx, dense_ratio, verify, wide=False, slot=0):
    """every accelerator of replica `slot` against the reference, in the state the caller expects the replica to be in"""
    nt = ref.alphabet == 0
    a = ix.debug_accelerators(slot)
    state = dict(k=a["seed_k"], entry_bytes=a["seed_entry_bytes"], seed_pos=a["seed_pos"], extra=a["ctx_extra"], lcx=bool(a["lcx_inner"]),
                 dense_ratio=int(a["dense_ratio"]), text8=bool(a["text8"]), text4=bool(a["text4"]))
    assert state == dict(k=k, entry_bytes=16 if wide else 8, seed_pos=int(seed_pos), extra=extra, lcx=lcx, dense_ratio=dense_ratio, text8=verify,
                         text4=verify and nt), (what, state)
    assert ix.seed_kmer_len() == k and ix.lcx_enabled() == lcx and ix.verify_enabled() == verify, what
    # the seed table
    T = ref.table(k, seed_pos, extra, lcx, wide)
    got = ix.debug_seed_table(slot)
    assert got.shape == T.entries.shape and got.dtype == T.entries.dtype, what
    bad = T.differences(got)
    assert len(bad) == 0, "%s: %d of %d seed entries differ; the first: %s" % (what, len(bad), len(got), T.explain(got, int(bad[0])))
    assert np.array_equal(T.masked(got), T.entries), what
    if lcx:
        assert not (got["cnt"][T.rows >= 2] & np.uint32(ar.SEED_LCX_NONE)).any(), what
    elif nt and not wide:
        assert not (got["cnt"][T.rows >= 2] >> np.uint32(29)).any(), what
    # the dense SA
    if dense_ratio:
        d, r = ix.debug_dense_sa(slot)
        assert r == dense_ratio == ix.locate_sa_ratio(), what
        same(d, ref.dense_sa(r), "%s: dense SA at ratio %d" % (what, r), r)
    else:
        assert ix.debug_dense_sa(slot) is None and not a["dense_sa"], what
    # the text
    if verify:
        same(ix.dev_download(a["text8"], (ref.n,), np.uint8, slot), ref.text8(), what + ": text8")
        if nt:
            assert a["text4_words"] == ref.text4_words(), what
            same(ix.dev_download(a["text4"], (ref.text4_words(),), np.uint32, slot), ref.text4(), what + ": text4", 8)
    # the SA of the N block
    lo, hi = ref.nblock_window()
    if nt and not wide and dense_ratio != 1 and hi - lo >= 64:
        assert a["sa_nblock"] and (a["nblock_lo"], a["nblock_hi"]) == (lo, hi), (what, a["nblock_lo"], a["nblock_hi"], lo, hi)
        same(ix.dev_download(a["sa_nblock"], (hi - lo,), np.uint32, slot), ref.sa_nblock(), what + ": sa_nblock")
    else:
        assert not a["sa_nblock"] and (a["nblock_lo"], a["nblock_hi"]) == (0, 0), what
    # the sampled levels of the left-context index
    if lcx:
        keys, _ = ix.debug_lcx(slot)
        levels, total = ref.lcx_levels()
        assert a["lcx_inner_words"] == total and a["lcx_off"][1:] == [off for off, _ in levels[1:]], (what, a["lcx_off"], levels)
        inner = ix.dev_download(a["lcx_inner"], (total,), np.uint64, slot)
        for t in range(1, 8):
            off, cnt = levels[t]
            same(inner[off:off + cnt], ref.lcx_inner_level(keys, t), "%s: lcx_inner level %d" % (what, t), 16 ** t)
    else:
        assert ix.debug_lcx(slot) is None and a["lcx_inner_words"] == 0, what


def nt_categories(ref, k, extra):
    """what the position-seed table of (k, E) holds, from the reference alone"""
    T = ref.table(k, True, extra, k >= 8)
    single, clen = T.rows == 1, ar.SEED_CTX_LEN + extra
    return dict(with_context=int((single & T.has_ctx).sum()), early=int((single & (T.pos < clen)).sum()),
                other_letter=int((single & ~T.has_ctx & (T.pos >= clen)).sum()), multi=int((T.rows >= 2).sum()),
                largest=int(T.rows.max()), tails=int(T.tail.sum()))


def assert_populated(name, ref, k, extra):
    c = nt_categories(ref, k, extra)
    if name == "family":
        assert c["multi"] >= 1000 and c["largest"] > 300 and c["tails"] >= 1, c
    else:
        assert c["with_context"] >= 4000 and c["early"] >= 10 and c["other_letter"] >= 50 and c["multi"] >= 150, (name, c)
    return c


def assert_amino_populated(ref, k):
    T = ref.table(k, True)
    single = T.rows == 1
    digits = np.arange(len(T.rows))
    has_x = np.zeros(len(T.rows), bool)
    for _ in range(k):
        has_x |= digits % 21 == 20
        digits //= 21
    c = dict(plain=int((T.rows >= 5).sum()), two=int((T.rows == 2).sum()), three=int((T.rows == 3).sum()), four=int((T.rows == 4).sum()),
             context=int((single & T.has_ctx).sum()), early=int((single & (T.pos < 6)).sum()), with_x=int((T.defined & has_x).sum()))
    assert all(v >= 1 for v in c.values()), c


def default_replica(name):
    text, st, hd, ref = world(name)
    k, extra = DEFAULT_K_E[name]
    assert ar.expected_ctx_extra(ref.n) == extra
    assert_populated(name, ref, k, extra)
    ix = FmIndex.from_text(text, 0, 8, 0, st, hd).set_devices([0])
    try:
        audit(ix, ref, "default replica of " + name, k, True, extra, True, 1, True)
    finally:
        ix.close()


# ---- 1. the default replica -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["5k", "20k", "90k", "family"])
def test_the_default_replica_is_the_text_s(name):
    """position seeds with their contexts and the left-context index's flags, the ratio-1 dense SA, text4, text8, lcx_inner"""
    default_replica(name)


# ---- 2. fewer context letters than a text of test size gets: the E of chr1 and GRCh38 scale -------------------------------------------
def counts_of(ix, q2d):
    if q2d.shape[1] <= 32:
        return ix.count_kmers_nt2(q2d, True)
    return np.diff(ix.locate_reads_nt2(q2d)[0])  # (33 letters: the packed reads kernels, with the table on as well)


@pytest.mark.parametrize("name", ["20k", "90k"])
def test_tables_of_fewer_context_letters_and_the_lengths_their_entries_decide(oracle, name):
    """E capped at 0, 1, 2, 3 (the clen <= 16 arithmetic of seed_rows_to_positions_kernel) and uncapped: the table, then on the
    same replica the counts of present, one-substitution and random L-mers, L = k + 14 + E - 1, + 0, + 1: around the length
    at which the entry alone decides"""
    text, st, hd, ref = world(name)
    k, full = DEFAULT_K_E[name]
    oi = oracle.OracleIndex.from_text(text, 0, 8, 0, st, hd)
    ix = FmIndex.from_text(text, 0, 8, 0, st, hd)
    rng = np.random.default_rng(k)
    try:
        for cap in (0, 1, 2, 3, -1):
            extra = ar.expected_ctx_extra(ref.n, cap)
            assert extra == (full if cap < 0 else cap)
            assert_populated(name, ref, k, extra)
            with ctx_extra_cap(cap):
                ix.set_devices([0])
            what = "%s, cap %d" % (name, cap)
            audit(ix, ref, what, k, True, extra, True, 1, True)
            for d in (-1, 0, 1):
                L = k + ar.SEED_CTX_LEN + extra + d
                pres = synth.sampled_queries(text, 2000, L, 100 + L)
                near = pres.copy()
                col = rng.integers(0, L, size=len(near))
                near[np.arange(len(near)), col] = synth.NT[(np.searchsorted(synth.NT, near[np.arange(len(near)), col]) + rng.integers(1, 4, size=len(near))) % 4]
                q2d = np.concatenate([pres, near, synth.random_queries(2000, L, 0, 200 + L)])
                qb, qo = synth.fixed_to_csr(q2d)
                want, _ = oi.parallel_count(qb, qo, 4)
                assert (want[:2000] >= 1).all() and (want[2000:4000] == 0).sum() > 1000
                got = counts_of(ix, q2d)
                assert np.array_equal(got, want), (what, L, "packed", np.flatnonzero(got != want)[:5])
                got = ix.parallel_count_csr(qb, qo)
                assert np.array_equal(got, want), (what, L, "host batch", np.flatnonzero(got != want)[:5])
    finally:
        L_.awry_debug_set_ctx_extra_cap(-1)
        ix.close()
        oi.close()


# ---- 3. what the table holds after every knob --------------------------------------------------------------------------------------
def test_the_table_after_every_transition():
    text, st, hd, ref = world("5k")
    k, extra = DEFAULT_K_E["5k"]
    assert 4 ** (k - 1) // 3 >= ref.n > 4 ** (k - 2) // 3  # position seeds are kept down to k - 1 = 7, below the left-context index's minimum of 8
    lo, hi = ref.nblock_window()
    assert hi - lo >= 64
    ix = FmIndex.from_text(text, 0, 8, 0, st, hd).set_devices([0])
    pos = dict(seed_pos=True, extra=extra, dense_ratio=1, verify=True)
    rows = dict(seed_pos=False, extra=0, lcx=False)
    try:
        audit(ix, ref, "default", k, lcx=True, **pos)
        ix.set_lcx(False)
        audit(ix, ref, "set_lcx(0)", k, lcx=False, **pos)
        ix.set_lcx(True)
        audit(ix, ref, "set_lcx(1)", k, lcx=True, **pos)
        ix.set_verify(-1)
        audit(ix, ref, "set_verify(-1)", k, dense_ratio=1, verify=False, **rows)
        ix.set_verify(2)
        audit(ix, ref, "set_verify(2)", k, lcx=True, **pos)
        ix.set_locate_sa_ratio(3)
        audit(ix, ref, "set_locate_sa_ratio(3)", k, dense_ratio=3, verify=False, **rows)
        ix.set_locate_sa_ratio(0)
        audit(ix, ref, "set_locate_sa_ratio(0)", k, dense_ratio=0, verify=False, **rows)
        ix.set_verify(2)
        audit(ix, ref, "set_verify(2) after set_locate_sa_ratio(0)", k, lcx=True, **pos)
        ix.set_seed_kmer_len(k - 1)
        audit(ix, ref, "set_seed_kmer_len(k - 1)", k - 1, lcx=False, **pos)
        ix.set_seed_kmer_len(8)
        audit(ix, ref, "set_seed_kmer_len(8)", 8, lcx=True, **pos)
        ix.set_seed_kmer_len(6)  # too dense for position seeds
        audit(ix, ref, "set_seed_kmer_len(6)", 6, dense_ratio=1, verify=True, **rows)
        ix.set_seed_kmer_len(7)
        audit(ix, ref, "set_seed_kmer_len(7)", 7, lcx=False, **pos)
        ix.set_seed_kmer_len(-1)
        audit(ix, ref, "set_seed_kmer_len(-1)", k, lcx=True, **pos)
        ix.set_devices([0, 0])
        for slot in (0, 1):
            audit(ix, ref, "set_devices([0, 0]), slot %d" % slot, k, lcx=True, slot=slot, **pos)
    finally:
        ix.close()


# ---- 4. the dense SA and the N block -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("file_ratio", [8, 3, 1])
def test_the_dense_sa_at_every_ratio_and_the_n_block(file_ratio):
    text, st, hd, ref = world("20k")
    k = DEFAULT_K_E["20k"][0]
    lo, hi = ref.nblock_window()
    assert hi - lo >= 64
    ix = FmIndex.from_text(text, 0, file_ratio, 0, st, hd).set_devices([0])
    try:
        ix.set_verify(-1)
        for ratio in (1, 2, 3, 8, 5):
            ix.set_locate_sa_ratio(ratio)
            audit(ix, ref, "file ratio %d, dense ratio %d" % (file_ratio, ratio), k, False, 0, False, ratio, False)
            assert bool(ix.debug_accelerators()["sa_nblock"]) == (ratio != 1)
    finally:
        ix.close()


# ---- 5. wide rows ----------------------------------------------------------------------------------------------------------------------
def test_wide_row_tables():
    text, st, hd, ref = world("5k")
    ix = FmIndex.from_text(text, 0, 8, 0, st, hd)
    try:
        with wide_rows():
            ix.set_devices([0])
        for k in (1, 2, 3, 4, -1):
            ix.set_seed_kmer_len(k)
            kk = DEFAULT_K_E["5k"][0] if k < 0 else k
            T = ref.table(kk, wide=True)
            assert (T.rows >= 2).sum() >= 1 and (k > 0 or (T.rows == 1).sum() >= 1000)  # (the default k: singletons with their symbols)
            audit(ix, ref, "wide rows, k = %d" % kk, kk, False, 0, False, 0, False, wide=True)
    finally:
        L_.awry_debug_force_wide_rows(0)
        ix.close()


def test_a_knob_refused_on_wide_rows_leaves_what_is_held():
    """set_locate_sa_ratio and set_verify need 32-bit rows: on a wide-row replica each has dropped its accelerators (none were
    there) by the time it refuses, and what the kernels see must still be what is held -- no dense SA, no texts, the wide table"""
    text, st, hd, ref = world("5k")
    k = DEFAULT_K_E["5k"][0]
    ix = FmIndex.from_text(text, 0, 8, 0, st, hd)
    try:
        with wide_rows():
            ix.set_devices([0])
        q2d = synth.sampled_queries(text, 2000, 12, 12)
        before = ix.count_kmers_nt2(q2d, True)
        assert (before >= 1).all()
        audit(ix, ref, "wide rows", k, False, 0, False, 0, False, wide=True)
        for what, knob in (("set_locate_sa_ratio(2)", lambda: ix.set_locate_sa_ratio(2)), ("set_verify(2)", lambda: ix.set_verify(2))):
            with pytest.raises(awry_amd.fm_index.AwryError) as err:
                knob()
            assert err.value.code == awry_amd.fm_index.ERR_ARG, what
            a = ix.debug_accelerators()
            assert not a["dense_sa"] and a["dense_ratio"] == 0 and not a["text4"] and not a["text8"], (what, a)
            audit(ix, ref, "wide rows after " + what, k, False, 0, False, 0, False, wide=True)
            assert np.array_equal(ix.count_kmers_nt2(q2d, True), before), what
    finally:
        L_.awry_debug_force_wide_rows(0)
        ix.close()


# ---- 6. amino ------------------------------------------------------------------------------------------------------------------------------
def amino_tables():
    text, st, hd, ref = world("amino")
    kd = DEFAULT_K_E["amino"][0]
    assert_amino_populated(ref, kd)
    ix = FmIndex.from_text(text, 1, 8, 0, st, hd).set_devices([0])
    try:
        for mode in ("positions", "rows"):
            if mode == "rows":
                ix.set_verify(-1)
            for k in (1, 2, 3, -1):
                ix.set_seed_kmer_len(k)
                kk = kd if k < 0 else k
                audit(ix, ref, "amino %s, k = %d" % (mode, kk), kk, mode == "positions", 0, False, 1, mode == "positions")
    finally:
        ix.close()


def test_amino_tables_in_rows_and_positions():
    amino_tables()


# ---- 7. the rungs --------------------------------------------------------------------------------------------------------------------------
def test_rung_tables_are_row_tables_of_their_length():
    text, st, hd, ref = world("90k")
    k, extra = DEFAULT_K_E["90k"]
    ix = FmIndex.from_text(text, 0, 8, 0, st, hd).set_devices([0])

    def rungs(what):
        for L in (6, 8, 10):
            T = ref.table(L)
            got = ix.debug_seed_rung(L)
            bad = T.differences(got)
            assert len(bad) == 0, "%s: rung %d: %d entries differ; the first: %s" % (what, L, len(bad), T.explain(got, int(bad[0])))
            assert np.array_equal(T.masked(got), T.entries)

    try:
        assert ix.seed_kmer_len() == k and ix.debug_accelerators()["seed_pos"] == 1
        assert ix.debug_seed_rung(5) is None and ix.debug_seed_rung(17) is None
        rungs("first use")
        ix.set_verify(-1)
        assert ix.debug_accelerators()["seed_pos"] == 0
        rungs("main table in rows")
        ix.set_verify(2)
        audit(ix, ref, "positions again", k, True, extra, True, 1, True)
        rungs("main table in positions again")
    finally:
        ix.close()


# ---- 8. builders whose lanes take many entries each ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["5k", "20k", "90k", "family"])
def test_the_default_replica_built_by_one_block(name):
    with max_blocks(1):
        default_replica(name)


def test_amino_tables_built_by_one_block():
    with max_blocks(1):
        amino_tables()
