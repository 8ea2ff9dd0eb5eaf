"""Anchors on the GPU (awry_amd/csrc/kernels_anchor.hip.h) against the two references of tests/anchor_ref.py: the definition
run with string search on small texts, LF stepping through the oracle on a 2 Mbp text, and the oracle's locate lists of the
anchor substrings.  Results must not depend on the seed table, the accelerators, the row width, the number of replicas or the
hit capacity of the locate chunks."""
import os

import numpy as np
import pytest

from awry_amd.fm_index import ANCHOR_DTYPE, ERR_INVALID_QUERY, AwryError, FmIndex, pack_queries
from tests import anchor_ref as ar
from tests import synth

pytestmark = pytest.mark.gpu


class World:
    """a text with its GPU index, its oracle index and a cache of reference (a) per (query, skip)"""

    def __init__(self, oracle, text, st, hd, alphabet):
        self.text, self.st, self.alphabet = text, st, alphabet
        self.ix = FmIndex.from_text(text, alphabet, 8, 0, st, hd).set_devices([0])
        self.oi = oracle.OracleIndex.from_text(text, alphabet, 8, 0, st, hd)
        self.ctext = ar.canonical_text(text, alphabet)
        self._ref = {}

    def ref(self, q, skip):
        key = (bytes(q), skip)
        if key not in self._ref:
            self._ref[key] = ar.anchors_definition(self.ctext, self.oi, q, self.alphabet, 1, skip)
        return self._ref[key]

    def want(self, qs, min_len, skip):
        return ar.as_csr([[a for a in self.ref(q, skip) if a[1] >= min_len] for q in qs])


def planted(text, rng, L, nsub, letters):
    p = int(rng.integers(0, len(text) - 1 - L))
    q = bytearray(text[p:p + L])
    for _ in range(nsub):
        j = int(rng.integers(0, L))
        q[j] = int(letters[(int(np.nonzero(letters == q[j])[0][0]) + 1) % len(letters)]) if q[j] in bytes(letters) else int(letters[0])
    return bytes(q)


def nt_queries(w, ks, n_sampled=150, n_random=60, seed=3):
    """length 1, lengths around the seed lengths `ks`, whole matches, reads of 30..150 letters with 0..4 planted substitutions,
    random reads, windows across N runs and record joins, all-N, lowercase / U / IUPAC, and a query of absent letters only"""
    rng = np.random.default_rng(seed)
    text, st = w.text, w.st
    n = len(text) - 1
    qs = [b"A", b"c", b"N", b"T"]
    for k in ks:
        for L in (k - 1, k, k + 1):
            if L >= 1:
                qs += [planted(text, rng, L, 0, synth.NT), planted(text, rng, L, 1, synth.NT), bytes(synth.NT[rng.integers(0, 4, size=L)])]
    for L in (12, 30, 101, 150):
        qs.append(planted(text, rng, L, 0, synth.NT))  # whole-query matches
    for _ in range(n_sampled):
        qs.append(planted(text, rng, int(rng.integers(30, 151)), int(rng.integers(0, 5)), synth.NT))
    for _ in range(n_random):
        qs.append(bytes(synth.NT[rng.integers(0, 4, size=int(rng.integers(1, 121)))]))
    for s in st[1:]:  # across record joins
        qs.append(bytes(text[s - 20:s + 25]))
    nrun = np.nonzero(text[:-1] == ord("N"))[0]
    if len(nrun):
        p = int(nrun[len(nrun) // 2])
        qs += [bytes(text[max(0, p - 30):p + 30]), bytes(text[int(nrun[0]) - 25:int(nrun[0]) + 6]), bytes(text[int(nrun[-1]) - 3:int(nrun[-1]) + 40])]
    p = int(rng.integers(0, n - 60))
    qs += [b"N" * 7, b"NNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNN", bytes(text[p:p + 60]).lower(), bytes(text[p:p + 60]).replace(b"T", b"U"),
           bytes(text[p:p + 60]).replace(b"A", b"R", 2), b"ACGTRYKMSWBDHVN", b"acgtnnnnacgt"]
    return qs


def check(w, ix, qs, min_lens=(1, 12), skips=(0, 1)):
    qb, qo = pack_queries(qs)
    for skip in skips:
        for min_len in min_lens:
            off, an = ix.parallel_anchors_csr(qb, qo, min_len, skip)
            woff, wrows = w.want(qs, min_len, skip)
            assert an.dtype == ANCHOR_DTYPE
            assert np.array_equal(off, woff), (min_len, skip)
            assert np.array_equal(ar.got_as_rows(an), wrows), (min_len, skip)


@pytest.fixture(scope="module")
def nt(oracle):
    return World(oracle, *synth.make_text(40_000, 0, 21, 5, 0.03), 0)


@pytest.fixture(scope="module")
def nt_qs(nt):
    return nt_queries(nt, (6, nt.ix.seed_kmer_len()))


def test_nucleotide_anchors_equal_the_definition(nt, nt_qs):
    assert len(nt_qs) >= 200
    check(nt, nt.ix, nt_qs)
    # the figures the fixture was chosen for: reads with 3 substitutions are cut into several anchors, random reads into many
    rng = np.random.default_rng(8)
    reads = [planted(nt.text, rng, 101, 3, synth.NT) for _ in range(40)]
    per = [len(nt.ref(q, 0)) for q in reads]
    assert 5.0 < np.mean(per) < 6.0 and max(per) <= 7, per
    rnd = [len(nt.ref(bytes(synth.NT[rng.integers(0, 4, size=101)]), 0)) for _ in range(20)]
    assert 13.0 < np.mean(rnd) < 15.0 and max(rnd) <= 15, rnd


@pytest.mark.parametrize("n", [1, 257, 3000])
def test_batch_sizes(nt, nt_qs, n):
    short = [q for q in nt_qs if len(q) <= 110]
    check(nt, nt.ix, [short[(7 * i) % len(short)] for i in range(n)], min_lens=(1,), skips=(0,) if n == 3000 else (0, 1))


def test_text_without_n_and_amino(oracle):
    w = World(oracle, *synth.make_text(4_000, 0, 22, 1, 0.0), 0)
    assert b"N" not in w.ctext
    rng = np.random.default_rng(4)
    qs = [b"N", b"NNNN", b"NRYK", b"ACGNNACGT"] + [planted(w.text, rng, int(rng.integers(20, 90)), int(rng.integers(0, 4)), synth.NT) for _ in range(60)]
    q = bytearray(planted(w.text, rng, 80, 0, synth.NT))
    q[33] = ord("N")
    qs += [bytes(q), bytes(q[:34]), bytes(q[33:])]
    check(w, w.ix, qs)
    assert w.ix.anchors_string(b"NNNN") == [] and w.ix.anchors_string(b"RYKM", 1, 1) == []  # every letter absent
    a = World(oracle, *synth.make_text(6_000, 1, 23, 4, 0.01), 1)
    ka = a.ix.seed_kmer_len()
    aq = [b"W", b"X", b"mkvB", b"BZJUO", bytes(a.text[a.st[1] - 5:a.st[1] + 6])]
    for L in (1, 2, 3, ka - 1, ka, ka + 1, 8, 20, 45):
        if L >= 1:
            aq += [planted(a.text, rng, L, 0, synth.AA), planted(a.text, rng, L, 1 if L > 1 else 0, synth.AA), bytes(synth.AA[rng.integers(0, 20, size=L)])]
    aq += [planted(a.text, rng, int(rng.integers(10, 70)), int(rng.integers(0, 4)), synth.AA) for _ in range(60)]
    check(a, a.ix, aq, min_lens=(1, 4))
    base = a.ix.parallel_anchors_csr(*pack_queries(aq))
    for k in (0, 2):
        a.ix.set_seed_kmer_len(k)
        got = a.ix.parallel_anchors_csr(*pack_queries(aq))
        assert np.array_equal(got[0], base[0]) and np.array_equal(got[1], base[1]), k


def test_stepping_reference_on_a_2_mbp_text(oracle):
    text, st, hd = synth.make_text(2_000_000, 0, 24, 6, 0.01)
    ix = FmIndex.from_text(text, 0, 8, 0, st, hd).set_devices([0])
    oi = oracle.OracleIndex.from_text(text, 0, 8, 0, st, hd)
    rng = np.random.default_rng(5)
    qs = [planted(text, rng, 101, int(rng.integers(0, 4)), synth.NT) for _ in range(1900)] + [bytes(q) for q in synth.random_queries(100, 101, 0, 6)]
    qb, qo = pack_queries(qs)
    for min_len, skip in ((1, 0), (20, 1)):
        off, an = ix.parallel_anchors_csr(qb, qo, min_len, skip)
        woff, wrows = ar.as_csr([ar.anchors_stepping(oi, q, 0, min_len, skip) for q in qs])
        assert np.array_equal(off, woff) and np.array_equal(ar.got_as_rows(an), wrows), (min_len, skip)
    ix.close()


def test_locate_anchors_equals_the_oracle_lists_and_survives_the_split_path(nt, nt_qs):
    qs = nt_qs[::2]
    qb, qo = pack_queries(qs)
    for max_hits, min_len, skip in ((1, 1, 0), (50, 1, 0), (50, 12, 1)):
        per = [[a for a in nt.ref(q, skip) if a[1] >= min_len] for q in qs]
        woff, wrows = ar.as_csr(per)
        whoff, wg, wp = ar.locate_reference(nt.oi, qs, per, 0, max_hits)
        got = nt.ix.parallel_locate_anchors_csr(qb, qo, max_hits, min_len, skip)
        off, an, hoff, g, p = got
        assert np.array_equal(off, woff) and np.array_equal(ar.got_as_rows(an), wrows)
        assert np.array_equal(hoff, whoff) and np.array_equal(g, wg) and np.array_equal(p, wp), (max_hits, min_len, skip)
        capped = an["count"] > max_hits
        assert (capped.any() or min_len > 1) and np.all(np.diff(hoff.astype(np.int64))[capped] == 0)
        assert int(hoff[-1]) > 64
        os.environ["AWRY_ANCHOR_HIT_CAP"] = "64"  # chunks split until each fits (or holds one query)
        try:
            again = nt.ix.parallel_locate_anchors_csr(qb, qo, max_hits, min_len, skip)
            nopos = nt.ix.parallel_locate_anchors_csr(qb, qo, max_hits, min_len, skip, want_pos=False)
        finally:
            del os.environ["AWRY_ANCHOR_HIT_CAP"]
        assert all(np.array_equal(x, y) for x, y in zip(got, again))
        assert all(np.array_equal(x, y) for x, y in zip(got[:4], nopos[:4])) and nopos[4].shape == (0, 2)


def census(ix, qs, min_len=1, skip=0, slot=0):
    """the device form with the census -> (n_anchors, tally[3])"""
    qb, qo = pack_queries(qs)
    n = len(qs)
    d_q, d_o = ix.dev_upload(np.concatenate([qb, np.zeros(16, np.uint8)]), slot), ix.dev_upload(qo, slot)
    d_n, d_t = ix.dev_malloc(8 * n, slot), ix.dev_malloc(24, slot)
    try:
        ix.dev_memset(d_t, 0, 24, slot)
        ix.dev_anchors_tally(d_q, d_o, n, min_len, skip, d_n, d_t, slot=slot)
        ix.dev_synchronize(slot)
        return ix.dev_download(d_n, (n,), np.uint64, slot), ix.dev_download(d_t, (3,), np.uint64, slot)
    finally:
        for p in (d_q, d_o, d_n, d_t):
            ix.dev_free(p, slot)


def test_results_do_not_depend_on_table_accelerators_row_width_or_replicas(nt, nt_qs):
    import awry_amd
    qb, qo = pack_queries(nt_qs)
    text, st = nt.text, nt.st
    hd = ["r%d" % i for i in range(len(st))]

    def results(ix):
        return tuple(ix.parallel_anchors_csr(qb, qo, 1, 0)) + tuple(ix.parallel_anchors_csr(qb, qo, 12, 1)) + tuple(ix.parallel_locate_anchors_csr(qb, qo, 20, 5, 0))

    def same(a, b):
        return all(np.array_equal(x, y) for x, y in zip(a, b))

    ix = FmIndex.from_text(text, 0, 8, 0, st, hd).set_devices([0])
    base = results(ix)
    woff, wrows = nt.want(nt_qs, 1, 0)
    assert np.array_equal(base[0], woff) and np.array_equal(ar.got_as_rows(base[1]), wrows)
    total_len = int(base[1]["q_len"].astype(np.int64).sum())
    at_zero = int((base[1]["q_begin"] == 0).sum())
    probes = {}
    for name, knob in (("default", lambda: None), ("k0", lambda: ix.set_seed_kmer_len(0)), ("k6", lambda: ix.set_seed_kmer_len(6)),
                       ("k6 verify off", lambda: ix.set_verify(-1)), ("k6 lcx off", lambda: ix.set_lcx(False)), ("k6 verify on", lambda: ix.set_verify(2)),
                       ("k6 lcx on", lambda: ix.set_lcx(True)), ("dense sa", lambda: ix.set_locate_sa_ratio(1)), ("kdefault", lambda: ix.set_seed_kmer_len(-1))):
        knob()
        assert same(results(ix), base), name
        na, t = census(ix, nt_qs)
        k = ix.seed_kmer_len()
        probes[name] = int(t[1])
        assert np.array_equal(na, np.diff(base[0])), name
        assert int(t[2]) == int(base[0][-1]), name                     # anchors reported
        # Every letter of an anchor costs one step, except the first of an anchor that starts from a single letter and the k of
        # one that starts from a table entry; an anchor that does not reach letter 0 ends in one more step, the failed one.
        assert int(t[0]) == total_len - (int(t[2]) - int(t[1])) - int(t[1]) * k + (int(t[2]) - at_zero), name
    assert probes["k0"] == 0 and probes["k6"] > 0 and probes["k6 verify off"] > 0 and probes["k6 verify on"] > 0, probes
    ix.set_devices([0, 0])  # two replicas: shards stitched in query order
    assert same(results(ix), base)
    ix.close()
    L_ = awry_amd.load_library()
    L_.awry_debug_force_wide_rows(1)
    try:
        wide = FmIndex.from_text(text, 0, 8, 0, st, hd).set_devices([0])
    finally:
        L_.awry_debug_force_wide_rows(0)
    try:
        assert "wide" in wide.count_schedule(31)
        assert same(results(wide), base)
        assert int(census(wide, nt_qs)[1][1]) == 0  # wide-row replicas skip the table
    finally:
        wide.close()


def test_device_form_on_streams_with_rejected_queries(nt, nt_qs):
    import torch
    ix = nt.ix
    sets = [nt_qs[:120] + [b"AC$T", b"", bytes([65, 0x80, 67]), b"A#"] + nt_qs[120:200], nt_qs[100:] + [b"$"] + nt_qs[:50]]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    jobs = []
    try:
        for qs, s in zip(sets, streams):
            qb, qo = pack_queries(qs)
            n = len(qs)
            good = [i for i, q in enumerate(qs) if len(q) and not any(c in b"$#" or c >= 0x80 for c in q)]
            woff, wrows = nt.want([qs[i] for i in good], 1, 1)
            wn = np.zeros(n, np.uint64)
            wn[good] = np.diff(woff)
            cap = int(wn.sum()) + 4
            j = dict(n=n, s=s.cuda_stream, good=good, wn=wn, wrows=wrows, cap=cap, d_q=ix.dev_upload(np.concatenate([qb, np.zeros(16, np.uint8)])),
                     d_o=ix.dev_upload(qo), d_n=ix.dev_malloc(8 * n), d_off=ix.dev_malloc(8 * (n + 1)), d_scr=ix.dev_malloc(ix.dev_scan_scratch_bytes(n)),
                     d_st=ix.dev_malloc(n), d_a=ix.dev_malloc(24 * cap))
            ix.dev_memset(j["d_a"], 0xEE, 24 * cap)
            ix.dev_memset(j["d_st"], 0xEE, n)
            jobs.append(j)
        ix.dev_synchronize()
        for j in jobs:  # both streams hold their three launches before anything is waited for
            ix.dev_anchors(j["d_q"], j["d_o"], j["n"], 1, 1, j["d_n"], None, None, j["d_st"], j["s"])
            ix.dev_scan_counts(j["d_n"], j["n"], j["d_off"], j["d_scr"], j["s"])
            ix.dev_anchors(j["d_q"], j["d_o"], j["n"], 1, 1, None, j["d_off"], j["d_a"], None, j["s"])
        ix.dev_synchronize()
        for j in jobs:
            n = j["n"]
            na, off = ix.dev_download(j["d_n"], (n,), np.uint64), ix.dev_download(j["d_off"], (n + 1,), np.uint64)
            status = ix.dev_download(j["d_st"], (n,), np.uint8)
            raw = ix.dev_download(j["d_a"], (24 * j["cap"],), np.uint8)
            assert np.array_equal(na, j["wn"])
            assert np.array_equal(off[1:], np.cumsum(j["wn"], dtype=np.uint64)) and off[0] == 0
            bad = np.ones(n, bool)
            bad[j["good"]] = False
            assert np.all(status[~bad] == 0) and np.all(status[bad] != 0) and np.all(na[bad] == 0)
            tot = int(off[-1])
            assert np.array_equal(ar.got_as_rows(raw[:24 * tot].view(ANCHOR_DTYPE)), j["wrows"])
            assert np.all(raw[24 * tot:] == 0xEE)  # nothing written past the last record
    finally:
        for j in jobs:
            for key in ("d_q", "d_o", "d_n", "d_off", "d_scr", "d_st", "d_a"):
                ix.dev_free(j[key])


def test_a_query_that_occurs_is_one_anchor_with_the_rows_of_search_range(nt, nt_qs):
    qb, qo = pack_queries(nt_qs)
    counts = nt.ix.parallel_count_csr(qb, qo)
    assert 20 < int((counts > 0).sum()) < len(nt_qs)
    for skip in (0, 1):
        off, an = nt.ix.parallel_anchors_csr(qb, qo, 1, skip)
        for i in np.nonzero(counts > 0)[0]:
            a = an[off[i]:off[i + 1]]
            r = nt.ix.search_range(nt_qs[i])
            assert len(a) == 1 and int(a[0]["q_begin"]) == 0 and int(a[0]["q_len"]) == len(nt_qs[i])
            assert (int(a[0]["start_row"]), int(a[0]["start_row"] + a[0]["count"]) - 1) == (r.start_ptr, r.end_ptr) and int(a[0]["count"]) == int(counts[i])
        for i in np.nonzero(counts == 0)[0][:40]:
            a = an[off[i]:off[i + 1]]
            assert len(a) != 1 or int(a[0]["q_len"]) < len(nt_qs[i])
    assert nt.ix.parallel_anchors([nt_qs[10], nt_qs[11]], 1, 0) == [nt.ref(nt_qs[10], 0), nt.ref(nt_qs[11], 0)]
    assert nt.ix.anchors_string(nt_qs[12], 12, 1) == [a for a in nt.ref(nt_qs[12], 1) if a[1] >= 12]


def test_invalid_query_in_a_batch_is_rejected_and_out_pointers_stay(nt):
    import ctypes as C
    import awry_amd
    from awry_amd import _lib
    for bad in (b"AC$T", b"", b"A#", bytes([0x41, 0x80])):
        qb, qo = pack_queries([b"ACGT", bad, b"GGA"])
        for call in (lambda: nt.ix.parallel_anchors_csr(qb, qo), lambda: nt.ix.parallel_locate_anchors_csr(qb, qo, 10)):
            with pytest.raises(AwryError) as e:
                call()
            assert e.value.code == ERR_INVALID_QUERY, bad
    L = awry_amd.load_library()
    u64p = C.POINTER(C.c_uint64)
    off, an, hoff, hits, gp = u64p(), C.POINTER(_lib.Anchor)(), u64p(), C.POINTER(_lib.Pos)(), u64p()
    qb, qo = pack_queries([b"ACGT", b"AC$T"])
    rc = L.awry_locate_anchors_batch(nt.ix._h, qb.ctypes.data, qo.ctypes.data_as(u64p), 2, 1, 0, 10, C.byref(off), C.byref(an), C.byref(hoff), C.byref(hits), C.byref(gp))
    assert rc == ERR_INVALID_QUERY and not off and not an and not hoff and not hits and not gp
    assert nt.ix.anchors_string(b"ACGT") == nt.ref(b"ACGT", 0)  # and the index still answers
