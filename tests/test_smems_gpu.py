"""SMEMs on the GPU (awry_amd/csrc/kernels_smem.hip.h) against the two references of tests/smem_ref.py: the definition run with
string search on small texts, the oracle's count_string on a 2 Mbp text, and the oracle's locate lists of the reported
substrings.  Results must not depend on the forward form (suffix-array search or bisection over backward searches), the seed
table, the accelerators, the row width, the number of replicas or the hit capacity of the locate chunks."""
import os

import numpy as np
import pytest

from awry_amd.fm_index import ANCHOR_DTYPE, ERR_INVALID_QUERY, AwryError, FmIndex, pack_queries
from tests import anchor_ref as ar
from tests import smem_ref as sr
from tests import synth
from tests.test_anchors_gpu import nt_queries, planted

pytestmark = pytest.mark.gpu


class World:
    """a text with its GPU index, its oracle index and a cache of reference (a) per query"""

    def __init__(self, oracle, text, st, hd, alphabet):
        self.text, self.st, self.hd, self.alphabet = text, st, hd, alphabet
        self.ix = FmIndex.from_text(text, alphabet, 8, 0, st, hd).set_devices([0])
        self.oi = oracle.OracleIndex.from_text(text, alphabet, 8, 0, st, hd)
        self.ctext = ar.canonical_text(text, alphabet)
        self._ref = {}

    def ref(self, q):
        key = bytes(q)
        if key not in self._ref:
            self._ref[key] = sr.smems_definition(self.ctext, self.oi, q, self.alphabet, 1)
        return self._ref[key]

    def want(self, qs, min_len):
        return ar.as_csr([[a for a in self.ref(q) if a[1] >= min_len] for q in qs])


def check(w, ix, qs, min_lens=(1, 12)):
    qb, qo = pack_queries(qs)
    for min_len in min_lens:
        off, sm = ix.parallel_smems_csr(qb, qo, min_len)
        woff, wrows = w.want(qs, min_len)
        assert sm.dtype == ANCHOR_DTYPE
        assert np.array_equal(off, woff), min_len
        assert np.array_equal(ar.got_as_rows(sm), wrows), min_len


def check_both_forms(w, qs, min_lens=(1, 12)):
    """the replica as built runs the suffix-array form; without the verify accelerators it runs the bisection"""
    assert w.ix.verify_enabled()
    check(w, w.ix, qs, min_lens)
    w.ix.set_verify(-1)
    try:
        assert not w.ix.verify_enabled()
        check(w, w.ix, qs, min_lens)
    finally:
        w.ix.set_verify(2)


def longest_run(ctext, letter):
    best = cur = 0
    for c in ctext:
        cur = cur + 1 if c == letter else 0
        best = max(best, cur)
    return best


def with_substitutions(text, rng, L, rate):
    p = int(rng.integers(0, len(text) - 1 - L))
    q = bytearray(text[p:p + L])
    for j in np.nonzero(rng.random(L) < rate)[0]:
        q[j] = int(synth.NT[(int(np.nonzero(synth.NT == q[j])[0][0]) + 1) % 4]) if q[j] in b"ACGT" else ord("A")
    return bytes(q)


def edge_queries(w, seed=9):
    """what the anchor suite's shapes do not reach: the text's two ends under the comparison, a whole record, runs longer than
    any in the text of the smallest and of the largest present letter (the insertion point at either edge of a bucket), and
    long reads"""
    rng = np.random.default_rng(seed)
    text, st = w.text, w.st
    n = len(text) - 1
    rnd5 = lambda: bytes(synth.NT[rng.integers(0, 4, size=5)])
    present = sorted(set(w.ctext[:-1]))
    lo_letter, hi_letter = present[0], present[-1]
    assert (lo_letter, hi_letter) == (ord("A"), ord("T"))
    qs = [bytes(text[n - 40:n]) + rnd5(),            # the comparison of the text's last suffixes reaches '$'
          rnd5() + bytes(text[:40]),
          bytes(text[st[1]:st[2]]),                  # a whole record
          bytes([lo_letter]) * (longest_run(w.ctext, lo_letter) + 3),
          bytes([hi_letter]) * (longest_run(w.ctext, hi_letter) + 3),
          with_substitutions(text, rng, 1000, 0.01), with_substitutions(text, rng, 5000, 0.01)]
    return qs


# what the definition (tests/smem_ref.py) gives for the 40 reads of the first test: 15.55 SMEMs per read, at most 20; 2.775 of
# length >= 12, at most 4
FIXTURE = dict(all_lo=15.0, all_hi=16.0, all_max=20, long_lo=2.5, long_hi=3.0, long_max=4)


@pytest.fixture(scope="module")
def nt(oracle):
    return World(oracle, *synth.make_text(40_000, 0, 21, 5, 0.03), 0)


@pytest.fixture(scope="module")
def nt_qs(nt):
    return nt_queries(nt, (6, nt.ix.seed_kmer_len())) + edge_queries(nt)


def test_nucleotide_smems_equal_the_definition_in_both_forward_forms(nt, nt_qs):
    assert len(nt_qs) >= 200
    check_both_forms(nt, nt_qs)
    # the character of the fixture, from the definition: 101-bp reads with 3 substitutions have many short SMEMs, few long ones,
    # and their SMEMs are never their anchors
    rng = np.random.default_rng(8)
    reads = [planted(nt.text, rng, 101, 3, synth.NT) for _ in range(40)]
    per = [nt.ref(q) for q in reads]
    n_all, n_long = [len(a) for a in per], [sum(1 for x in a if x[1] >= 12) for a in per]
    print("SMEMs per read: mean %.2f max %d; of length >= 12: mean %.2f max %d" % (np.mean(n_all), max(n_all), np.mean(n_long), max(n_long)))
    assert FIXTURE["all_lo"] < np.mean(n_all) < FIXTURE["all_hi"] and max(n_all) <= FIXTURE["all_max"], n_all
    assert FIXTURE["long_lo"] < np.mean(n_long) < FIXTURE["long_hi"] and max(n_long) <= FIXTURE["long_max"], n_long
    for q, a in zip(reads, per):
        assert a != ar.anchors_definition(nt.ctext, nt.oi, q, 0, 1, 0), q
    check(nt, nt.ix, reads)


@pytest.mark.parametrize("n", [1, 257, 3000])
def test_batch_sizes(nt, nt_qs, n):
    short = [q for q in nt_qs if len(q) <= 110]
    check(nt, nt.ix, [short[(7 * i) % len(short)] for i in range(n)], min_lens=(1,))


def nfree_world(oracle, body):
    """a one-record nucleotide text of exactly these letters"""
    text = np.frombuffer(body + b"$", np.uint8).copy()
    return World(oracle, text, [0], ["r0"], 0)


def test_homopolymer_and_period(oracle):
    w = nfree_world(oracle, b"CG" + b"A" * 200 + b"CT" + b"A" * 50 + b"G")
    assert b"N" not in w.ctext
    want300 = [(b, 200, None, 1) for b in range(100, -1, -1)]
    for form in ("sa", "lf"):
        if form == "lf":
            w.ix.set_verify(-1)
        assert w.ix.verify_enabled() == (form == "sa")
        got = w.ix.smems_string(b"A" * 300)
        assert [(b, ln, c) for b, ln, _, c in got] == [(b, ln, c) for b, ln, _, c in want300], form
        assert got == w.ref(b"A" * 300)
        assert len(w.ix.smems_string(b"A" * 200)) == 1 and w.ix.smems_string(b"A" * 200) == w.ref(b"A" * 200)
        assert len(w.ix.smems_string(b"A" * 201)) == 2 and w.ix.smems_string(b"A" * 201) == w.ref(b"A" * 201)
        check(w, w.ix, [b"A" * 300, b"A" * 251, b"A" * 50 + b"G", b"T" + b"A" * 60, b"CG" + b"A" * 210, b"G" * 5, b"T" * 4], min_lens=(1, 12, 200, 201))
    w.ix.close()
    rng = np.random.default_rng(12)
    flank = lambda: bytes(synth.NT[rng.integers(0, 4, size=300)])
    p = nfree_world(oracle, flank() + b"ACGT" * 100 + flank())
    qs = [b"ACGT" * 120, b"CGTA" * 110 + b"C", b"ACGT" * 100, b"GT" + b"ACGT" * 99 + b"AC"]
    check_both_forms(p, qs, min_lens=(1, 12, 400))
    assert len(p.ref(b"ACGT" * 120)) >= 21  # the whole array at every begin in phase with it, 0, 4, .. 80
    p.ix.close()


def test_text_without_n_and_amino(oracle):
    w = World(oracle, *synth.make_text(4_000, 0, 22, 1, 0.0), 0)
    assert b"N" not in w.ctext
    rng = np.random.default_rng(4)
    qs = [b"N", b"NNNN", b"NRYK", b"ACGNNACGT"] + [planted(w.text, rng, int(rng.integers(20, 90)), int(rng.integers(0, 4)), synth.NT) for _ in range(60)]
    q = bytearray(planted(w.text, rng, 80, 0, synth.NT))
    q[33] = ord("N")
    qs += [bytes(q), bytes(q[:34]), bytes(q[33:])]
    check_both_forms(w, qs)
    assert w.ix.smems_string(b"NNNN") == [] and w.ix.smems_string(b"RYKM", 1) == []  # every letter absent
    assert [(b, ln) for b, ln, _, _ in w.ix.smems_string(bytes(q))] == [(34, 46), (0, 33)]  # an absent letter splits SMEMs
    w.ix.close()
    a = World(oracle, *synth.make_text(6_000, 1, 23, 4, 0.01), 1)
    ka = a.ix.seed_kmer_len()
    aq = [b"W", b"X", b"mkvB", b"BZJUO", bytes(a.text[a.st[1] - 5:a.st[1] + 6]), bytes(a.text[len(a.text) - 31:len(a.text) - 1]) + b"WW", bytes(a.text[a.st[2]:a.st[3]])]
    for L in (1, 2, 3, ka - 1, ka, ka + 1, 8, 20, 45):
        if L >= 1:
            aq += [planted(a.text, rng, L, 0, synth.AA), planted(a.text, rng, L, 1 if L > 1 else 0, synth.AA), bytes(synth.AA[rng.integers(0, 20, size=L)])]
    aq += [planted(a.text, rng, int(rng.integers(10, 70)), int(rng.integers(0, 4)), synth.AA) for _ in range(60)]
    check_both_forms(a, aq, min_lens=(1, 4))
    base = a.ix.parallel_smems_csr(*pack_queries(aq))
    for k in (0, 2, -1):
        a.ix.set_seed_kmer_len(k)
        got = a.ix.parallel_smems_csr(*pack_queries(aq))
        assert np.array_equal(got[0], base[0]) and np.array_equal(got[1], base[1]), k
    a.ix.close()


def census(ix, qs, min_len=1, slot=0):
    """the device form with the census -> (n_smems, tally[4])"""
    qb, qo = pack_queries(qs)
    n = len(qs)
    d_q, d_o = ix.dev_upload(np.concatenate([qb, np.zeros(16, np.uint8)]), slot), ix.dev_upload(qo, slot)
    d_n, d_t = ix.dev_malloc(8 * n, slot), ix.dev_malloc(32, slot)
    try:
        ix.dev_memset(d_t, 0, 32, slot)
        ix.dev_smems_tally(d_q, d_o, n, min_len, d_n, d_t, slot=slot)
        ix.dev_synchronize(slot)
        return ix.dev_download(d_n, (n,), np.uint64, slot), ix.dev_download(d_t, (4,), np.uint64, slot)
    finally:
        for p in (d_q, d_o, d_n, d_t):
            ix.dev_free(p, slot)


def test_results_do_not_depend_on_form_table_accelerators_row_width_or_replicas(nt, nt_qs):
    import awry_amd
    qb, qo = pack_queries(nt_qs)
    text, st = nt.text, nt.st
    hd = ["r%d" % i for i in range(len(st))]

    def results(ix):
        return tuple(ix.parallel_smems_csr(qb, qo, 1)) + tuple(ix.parallel_smems_csr(qb, qo, 12)) + tuple(ix.parallel_locate_smems_csr(qb, qo, 20, 5))

    def same(a, b):
        return all(np.array_equal(x, y) for x, y in zip(a, b))

    ix = FmIndex.from_text(text, 0, 8, 0, st, hd).set_devices([0])
    base = results(ix)
    woff, wrows = nt.want(nt_qs, 1)
    assert np.array_equal(base[0], woff) and np.array_equal(ar.got_as_rows(base[1]), wrows)
    n_all = int(base[0][-1])
    n12 = int(base[2][-1])
    # the k = 0 suffix-array form: every extension walks back from e -- e - b - 1 steps that commit and, unless b == 0, the one that fails
    steps_k0_sa = int((base[1]["q_len"].astype(np.int64) - 1).sum()) + int((base[1]["q_begin"] > 0).sum())
    sa_probes = {}
    for name, knob in (("default", lambda: None), ("k0", lambda: ix.set_seed_kmer_len(0)), ("k6", lambda: ix.set_seed_kmer_len(6)),
                       ("k6 verify off", lambda: ix.set_verify(-1)), ("k0 verify off", lambda: ix.set_seed_kmer_len(0)), ("k6 lcx off", lambda: (ix.set_seed_kmer_len(6), ix.set_lcx(False))),
                       ("k6 verify on", lambda: ix.set_verify(2)), ("k6 lcx on", lambda: ix.set_lcx(True)), ("dense sa", lambda: ix.set_locate_sa_ratio(1)),
                       ("verify again", lambda: ix.set_verify(2)), ("kdefault", lambda: ix.set_seed_kmer_len(-1))):
        knob()
        assert same(results(ix), base), name
        ns, t = census(ix, nt_qs)
        sa_probes[name] = int(t[1])
        assert (int(t[1]) > 0) == ix.verify_enabled(), name                # suffixes are compared exactly when the SA form runs
        assert np.array_equal(ns, np.diff(base[0])), name
        assert int(t[2]) == n_all and int(t[3]) == n_all, name               # extensions, records
        ns12, t12 = census(ix, nt_qs, 12)
        assert np.array_equal(ns12, np.diff(base[2])) and int(t12[3]) == n12 and int(t12[2]) == n_all and int(t12[0]) == int(t[0]), name
        if ix.seed_kmer_len() == 0 and ix.verify_enabled():
            assert int(t[0]) == steps_k0_sa, name
    assert sa_probes["default"] > 0 and sa_probes["k0"] > 0 and sa_probes["k6 verify on"] > 0 and sa_probes["verify again"] > 0, sa_probes
    assert sa_probes["k6 verify off"] == 0 and sa_probes["k0 verify off"] == 0 and sa_probes["k6 lcx off"] == 0, sa_probes
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
        ns, t = census(wide, nt_qs)
        assert int(t[1]) == 0 and int(t[2]) == n_all and int(t[3]) == n_all  # wide rows: the bisection, no suffix compared
    finally:
        wide.close()


def test_oracle_reference_on_a_2_mbp_text_in_both_forms(oracle):
    text, st, hd = synth.make_text(2_000_000, 0, 24, 6, 0.01)
    ix = FmIndex.from_text(text, 0, 8, 0, st, hd).set_devices([0])
    oi = oracle.OracleIndex.from_text(text, 0, 8, 0, st, hd)
    rng = np.random.default_rng(5)
    qs = [planted(text, rng, 101, int(rng.integers(0, 4)), synth.NT) for _ in range(400)] + [bytes(q) for q in synth.random_queries(50, 101, 0, 6)]
    qb, qo = pack_queries(qs)
    ref = [sr.smems_oracle(oi, q, 0, 1) for q in qs]
    for form in ("sa", "lf"):
        if form == "lf":
            ix.set_verify(-1)
        assert ix.verify_enabled() == (form == "sa")
        for min_len in (1, 20):
            off, sm = ix.parallel_smems_csr(qb, qo, min_len)
            woff, wrows = ar.as_csr([[a for a in r if a[1] >= min_len] for r in ref])
            assert np.array_equal(off, woff) and np.array_equal(ar.got_as_rows(sm), wrows), (form, min_len)
    ix.close()


def test_locate_smems_equals_the_oracle_lists_and_survives_the_split_path(nt, nt_qs):
    qs = [q for q in nt_qs[::2] if len(q) <= 1000]
    qb, qo = pack_queries(qs)
    for max_hits, min_len in ((1, 1), (50, 1), (50, 12)):
        per = [[a for a in nt.ref(q) if a[1] >= min_len] for q in qs]
        woff, wrows = ar.as_csr(per)
        whoff, wg, wp = ar.locate_reference(nt.oi, qs, per, 0, max_hits)
        got = nt.ix.parallel_locate_smems_csr(qb, qo, max_hits, min_len)
        off, sm, hoff, g, p = got
        assert np.array_equal(off, woff) and np.array_equal(ar.got_as_rows(sm), wrows)
        assert np.array_equal(hoff, whoff) and np.array_equal(g, wg) and np.array_equal(p, wp), (max_hits, min_len)
        capped = sm["count"] > max_hits
        assert (capped.any() or min_len > 1) and np.all(np.diff(hoff.astype(np.int64))[capped] == 0)  # capped records keep no hits
        assert int(hoff[-1]) > 64
        os.environ["AWRY_ANCHOR_HIT_CAP"] = "64"  # chunks split until each fits (or holds one query)
        try:
            again = nt.ix.parallel_locate_smems_csr(qb, qo, max_hits, min_len)
            nopos = nt.ix.parallel_locate_smems_csr(qb, qo, max_hits, min_len, want_pos=False)
        finally:
            del os.environ["AWRY_ANCHOR_HIT_CAP"]
        assert all(np.array_equal(x, y) for x, y in zip(got, again))
        assert all(np.array_equal(x, y) for x, y in zip(got[:4], nopos[:4])) and nopos[4].shape == (0, 2)


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
            woff, wrows = nt.want([qs[i] for i in good], 1)
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
            ix.dev_smems(j["d_q"], j["d_o"], j["n"], 1, j["d_n"], None, None, j["d_st"], j["s"])
            ix.dev_scan_counts(j["d_n"], j["n"], j["d_off"], j["d_scr"], j["s"])
            ix.dev_smems(j["d_q"], j["d_o"], j["n"], 1, None, j["d_off"], j["d_a"], None, j["s"])
        ix.dev_synchronize()
        for j in jobs:
            n = j["n"]
            ns, off = ix.dev_download(j["d_n"], (n,), np.uint64), ix.dev_download(j["d_off"], (n + 1,), np.uint64)
            status = ix.dev_download(j["d_st"], (n,), np.uint8)
            raw = ix.dev_download(j["d_a"], (24 * j["cap"],), np.uint8)
            assert np.array_equal(ns, j["wn"])
            assert np.array_equal(off[1:], np.cumsum(j["wn"], dtype=np.uint64)) and off[0] == 0
            bad = np.ones(n, bool)
            bad[j["good"]] = False
            assert np.all(status[~bad] == 0) and np.all(status[bad] != 0) and np.all(ns[bad] == 0)
            tot = int(off[-1])
            assert np.array_equal(ar.got_as_rows(raw[:24 * tot].view(ANCHOR_DTYPE)), j["wrows"])
            assert np.all(raw[24 * tot:] == 0xEE)  # nothing written past the last record
    finally:
        for j in jobs:
            for key in ("d_q", "d_o", "d_n", "d_off", "d_scr", "d_st", "d_a"):
                ix.dev_free(j[key])


def test_a_query_that_occurs_is_one_smem_and_the_first_smem_is_the_first_anchor(nt, nt_qs):
    qb, qo = pack_queries(nt_qs)
    counts = nt.ix.parallel_count_csr(qb, qo)
    assert 20 < int((counts > 0).sum()) < len(nt_qs)
    off, sm = nt.ix.parallel_smems_csr(qb, qo, 1)
    aoff, an = nt.ix.parallel_anchors_csr(qb, qo, 1, 0)
    for i in np.nonzero(counts > 0)[0]:
        a = sm[off[i]:off[i + 1]]
        r = nt.ix.search_range(nt_qs[i])
        assert len(a) == 1 and int(a[0]["q_begin"]) == 0 and int(a[0]["q_len"]) == len(nt_qs[i])
        assert (int(a[0]["start_row"]), int(a[0]["start_row"] + a[0]["count"]) - 1) == (r.start_ptr, r.end_ptr) and int(a[0]["count"]) == int(counts[i])
    for i in np.nonzero(counts == 0)[0][:40]:
        a = sm[off[i]:off[i + 1]]
        assert len(a) != 1 or int(a[0]["q_len"]) < len(nt_qs[i])
    for i in range(len(nt_qs)):
        assert (off[i + 1] > off[i]) == (aoff[i + 1] > aoff[i])
        if off[i + 1] > off[i]:
            assert sm[off[i]] == an[aoff[i]], i
    assert nt.ix.parallel_smems([nt_qs[10], nt_qs[11]], 1) == [nt.ref(nt_qs[10]), nt.ref(nt_qs[11])]
    assert nt.ix.smems_string(nt_qs[12], 12) == [a for a in nt.ref(nt_qs[12]) if a[1] >= 12]


def test_invalid_query_in_a_batch_is_rejected_and_out_pointers_stay(nt):
    import ctypes as C
    import awry_amd
    from awry_amd import _lib
    for bad in (b"AC$T", b"", b"A#", bytes([0x41, 0x80])):
        qb, qo = pack_queries([b"ACGT", bad, b"GGA"])
        for call in (lambda: nt.ix.parallel_smems_csr(qb, qo), lambda: nt.ix.parallel_locate_smems_csr(qb, qo, 10)):
            with pytest.raises(AwryError) as e:
                call()
            assert e.value.code == ERR_INVALID_QUERY, bad
    L = awry_amd.load_library()
    u64p = C.POINTER(C.c_uint64)
    off, sm, hoff, hits, gp = u64p(), C.POINTER(_lib.Anchor)(), u64p(), C.POINTER(_lib.Pos)(), u64p()
    qb, qo = pack_queries([b"ACGT", b"AC$T"])
    rc = L.awry_locate_smems_batch(nt.ix._h, qb.ctypes.data, qo.ctypes.data_as(u64p), 2, 1, 10, C.byref(off), C.byref(sm), C.byref(hoff), C.byref(hits), C.byref(gp))
    assert rc == ERR_INVALID_QUERY and not off and not sm and not hoff and not hits and not gp
    assert nt.ix.smems_string(b"ACGT") == nt.ref(b"ACGT")  # and the index still answers


# ---- small batches through the chunk driver's rarely taken branches (shared with the chain, align-chains and map suites) ---------

def small_reads(w, n=64, L=101, seed=123):
    """n reads of L letters out of the text, free of N: every fourth is two halves from two places (two chains), every other of the
    rest has one substitution in the middle (two SMEMs)"""
    rng = np.random.default_rng(seed)
    text = bytes(w.text)
    out = []
    while len(out) < n:
        p, p2 = (int(x) for x in rng.integers(0, len(text) - 1 - L, size=2))
        q = bytearray(text[p:p + L] if len(out) % 4 else text[p:p + 50] + text[p2:p2 + L - 50])
        if len(out) % 4 == 2:
            q[L // 2] = b"ACGT"[(b"ACGT".index(q[L // 2]) + 1) % 4] if q[L // 2] in b"ACGT" else 0
        if all(c in b"ACGT" for c in q):
            out.append(bytes(q))
    return out


class shrunk_cap:
    """with shrunk_cap("AWRY_ANCHOR_HIT_CAP"): every chunk of more than one read is over capacity and halves down to single reads"""

    def __init__(self, *names):
        self.names = names

    def __enter__(self):
        for k in self.names:
            os.environ[k] = "1"

    def __exit__(self, *exc):
        for k in self.names:
            del os.environ[k]


def with_bad_read(reads, bad):
    """7 reads with `bad` in the middle"""
    return reads[:3] + [bad] + reads[3:6]


def all_equal(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and np.array_equal(x, y) for x, y in zip(a, b))


def test_a_chunk_without_smems_gives_zero_offsets(nt):
    reads = small_reads(nt)
    off, sm, hoff, g, p = nt.ix.parallel_locate_smems_csr(*pack_queries(reads), 50, 102)  # min_len above every read's length
    assert np.array_equal(off, np.zeros(len(reads) + 1, np.uint64)) and len(sm) == 0
    assert np.array_equal(hoff, [0]) and len(g) == 0 and p.shape == (0, 2)


def test_a_bad_read_is_named_before_the_capacity_test_splits_its_chunk(nt):
    reads = small_reads(nt, 6)
    assert int(nt.ix.parallel_locate_smems_csr(*pack_queries(reads), 50, 12)[2][-1]) > 6  # over a capacity of one hit
    with shrunk_cap("AWRY_ANCHOR_HIT_CAP"):
        for bad in (b"AC$T", b"", bytes([0x41, 0x80])):
            with pytest.raises(AwryError) as e:
                nt.ix.parallel_locate_smems_csr(*pack_queries(with_bad_read(reads, bad)), 50, 12)
            assert e.value.code == ERR_INVALID_QUERY and "query 3:" in str(e.value), bad


def test_seven_reads_halved_down_to_single_reads_equal_the_uncapped_call(nt):
    reads = small_reads(nt, 7)
    qb, qo = pack_queries(reads)
    want = nt.ix.parallel_locate_smems_csr(qb, qo, 50, 12), nt.ix.parallel_locate_anchors_csr(qb, qo, 50, 12)
    assert all(int(w[2][-1]) > 7 for w in want)
    with shrunk_cap("AWRY_ANCHOR_HIT_CAP"):
        got = nt.ix.parallel_locate_smems_csr(qb, qo, 50, 12), nt.ix.parallel_locate_anchors_csr(qb, qo, 50, 12)
    assert all_equal(want[0], got[0]) and all_equal(want[1], got[1])
