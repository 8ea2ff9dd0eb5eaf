"""GPU audit of the k-mer count table (awry_amd/csrc/kmer_table.hip.h, mode 7 of resume_block_list, accelerators.h): the table
itself, read with FmIndex.debug_kmer_table(), against a host recomputation from the text (tests/kmer_table_ref.py).

A miss in a line that is not marked overflowed is answered "count 0" with no search behind it, so the table must hold every
distinct L-mer of every covered bucket with exactly its count; tests/test_kmer_table_gpu.py sees it only through a few thousand
queries.  Here: the whole table at the policy size, half full, with tags too wide for its line bits, with a count field at and
around its saturation value, replaced while launches of another length are in flight, and across what drops and rebuilds it.
Nothing here has a tolerance: the reference determines the table up to which 16 keys a full line keeps.

Census word 6 counts index lines: one per table line read, one per line of a search.  A query whose seed bucket has more
than 4 rows goes to the table (1 line); it is searched behind that (1 line or more) iff its line does not settle it."""
import threading
import time

import numpy as np
import pytest

from awry_amd import _lib
from awry_amd.fm_index import FmIndex
from tests import kmer_table_ref as ref
from tests import synth
from tests.test_kmer_table_gpu import census_run, check_counts, world  # noqa: F401  (world: the module fixture, one instance for this module)

pytestmark = pytest.mark.gpu

_REFS = {}


def world_ref(w, L, k=None):
    """reference_table of the World text for (seed length, L), computed once"""
    k = w.k if k is None else k
    if (k, L) not in _REFS:
        _REFS[(k, L)] = ref.reference_table(w.text, k, L)
    return _REFS[(k, L)]


def unpack(words, L):
    """uint64[n] packed L-mers -> uint8[n, L] ASCII"""
    return synth.NT[((np.asarray(words, np.uint64)[:, None] >> (2 * np.arange(L, dtype=np.uint64))[None, :]) & np.uint64(3)).astype(np.int64)]


def lookup(words, counts, q):
    """counts of the packed queries q by the sorted reference (words, counts); 0 where it does not hold them"""
    if len(words) == 0:
        return np.zeros(len(q), np.uint64)
    at = np.minimum(np.searchsorted(words, q), len(words) - 1)
    return np.where(words[at] == q, counts[at], 0).astype(np.uint64)


def substituted_head(q2d, head, rng):
    """one substitution per k-mer among its first `head` letters (as substituted() of test_kmer_table_gpu.py, but the last k
    letters -- the seed bucket, and with it whether the query goes to the table -- stay)"""
    near = q2d.copy()
    col = rng.integers(0, head, size=len(near))
    rows = np.arange(len(near))
    near[rows, col] = synth.NT[(np.searchsorted(synth.NT[:4], near[rows, col]) + 1 + rng.integers(0, 3, size=len(near))) % 4]
    return near


def fresh_table(ix, L, q2d):
    """drops the table, then builds the one of length L with ONE launch of a few k-mers -> (table, bits, info)"""
    ix.set_kmer_table(0)
    ix.set_kmer_table(1)
    assert ix.kmer_table_info()["length"] == 0 and ix.debug_kmer_table() is None
    ix.count_kmers_nt2(np.ascontiguousarray(q2d[:100]), True)
    return read_table(ix, L)


def read_table(ix, L):
    got = ix.debug_kmer_table()
    assert got is not None, "no table resident"
    tab, bits, Lt = got
    info = ix.kmer_table_info()
    assert Lt == L == info["length"] and info["lines"] == 1 << bits and len(tab) == 16 << bits, (L, Lt, bits, info)
    return tab, bits, info


def audit_resident(ix, L, words, counts):
    tab, bits, info = read_table(ix, L)
    entries, marked = ref.audit(tab, bits, L, words, counts)
    assert info["entries"] == entries and info["overflowed_lines"] == marked, (info, entries, marked)
    return tab, bits, info


def forced_lines(lines):
    class Forced:
        def __enter__(self):
            _lib.load_library().awry_debug_set_kmer_table_lines(lines)

        def __exit__(self, *exc):
            _lib.load_library().awry_debug_set_kmer_table_lines(0)
    return Forced()


def test_packing_is_dev_pack_nt2_s(world):
    """the reference packs a k-mer as the device does: first letter least significant"""
    w = world
    for L in (w.k + 1, 21, 31, 32):
        q2d = w.batch(L)[0][:1000]
        n = len(q2d)
        d_ascii = w.ix.dev_upload(np.ascontiguousarray(q2d).reshape(-1))
        d_words, d_bad = w.ix.dev_malloc(8 * n), w.ix.dev_malloc(8)
        try:
            w.ix.dev_memset(d_bad, 0, 8)
            w.ix.dev_pack_nt2(d_ascii, n, L, d_words, d_bad)
            w.ix.dev_synchronize()
            assert int(w.ix.dev_download(d_bad, (1,), np.uint64)[0]) == 0
            assert np.array_equal(w.ix.dev_download(d_words, (n,), np.uint64), ref.pack_queries(q2d)), L
        finally:
            for p in (d_ascii, d_words, d_bad):
                w.ix.dev_free(p)
        assert np.array_equal(unpack(ref.pack_queries(q2d), L), q2d)


@pytest.mark.parametrize("L", [31, 21, 32, "k+1"])
def test_the_table_of_the_policy_s_size_is_the_text_s(world, L):
    """(a) every distinct L-mer of every bucket of more than 4 rows, exactly its count, nothing else, marks where they belong.
    Not vacuous: more than 100 000 keys for L = 31, 21, 32.  For L = k + 1 that number is out of reach of this text whatever
    the table does -- a key is a covered k-mer with one letter in front, the text has 37 391 of them (k = 13) -- so there the
    audit must cover at least one key per covered k-mer, and more than 10 000 of those."""
    w = world
    L = w.k + 1 if L == "k+1" else L
    words, counts = world_ref(w, L)
    if L == w.k + 1:
        kw, kc = ref.kmer_counts(w.text, w.k)
        assert len(words) >= int((kc > ref.LANE_ROWS).sum()) > 10_000, (len(words), int((kc > ref.LANE_ROWS).sum()))
    else:
        assert len(words) > 100_000, len(words)
    tab, bits, info = fresh_table(w.ix, L, w.batch(L)[0])
    entries, marked = ref.audit(tab, bits, L, words, counts)
    print("L = %d: %d reference keys, max count %d; table of 2^%d lines, %d entries, %d marked" % (L, len(words), int(counts.max()), bits, entries, marked))
    assert info["entries"] == entries and info["overflowed_lines"] == marked and info["lines"] == 1 << bits, (info, entries, marked)
    w.ix.set_kmer_table(0)


def half_full_bits(words, L):
    """the table sizes (log2 lines) at which between 20 % and 80 % of the lines get more than 16 keys, from the reference alone"""
    out = []
    for bits in range(4, 26):
        _, _, storable, n_store, _ = ref.expected_lines(words, L, bits)
        share = float((n_store > 16).mean())
        if storable.all() and 0.20 <= share <= 0.80:
            out.append((bits, share))
    return out


@pytest.mark.parametrize("L", [21, "k+1"])
def test_a_half_full_table(world, L):
    """(b) some lines full and some not: a miss in an unmarked line is 0 from one line, a miss in a marked one is searched"""
    w = world
    L = w.k + 1 if L == "k+1" else L
    words, counts = world_ref(w, L)
    sizes = half_full_bits(words, L)
    assert sizes, "no power of two of lines leaves 20 .. 80 % of the lines full for this text"
    bits, share = sizes[0]
    rng = np.random.default_rng(200 + L)
    with forced_lines(1 << bits):
        try:
            tab, got_bits, info = fresh_table(w.ix, L, w.batch(L)[0])
            assert got_bits == bits
            problems = []  # (the audit and the counts are judged together: a table that is wrong shows in both)
            try:
                entries, n_marked = ref.audit(tab, bits, L, words, counts)
                assert info["entries"] == entries and info["overflowed_lines"] == n_marked, (info, entries, n_marked)
                print("L = %d: %d keys forced into 2^%d lines, predicted share of full lines %.3f; %d entries, %d marked" % (L, len(words), bits, share, entries, n_marked))
            except AssertionError as e:
                problems.append(("audit", e.args))
            # every reference key (or 200 000 of them), and as many k-mers one substitution away: all go to the table
            pick = np.arange(len(words)) if len(words) <= 200_000 else rng.choice(len(words), size=200_000, replace=False)
            pres_w = words[pick]
            pres = unpack(pres_w, L)
            near = substituted_head(pres, L - w.k, rng)
            near_w = ref.pack_queries(near)
            q2d = np.concatenate([pres, near])
            qw = np.concatenate([pres_w, near_w])
            want = lookup(words, counts, qw)  # (the bucket of every query is covered: the reference holds all its L-mers)
            assert (want[:len(pres)] > 0).all() and (want[len(pres):] == 0).mean() > 0.5
            got, census = census_run(w.ix, q2d)
            bad = np.flatnonzero(got != want)
            if len(bad):
                problems.append(("counts: wrong, first indices, got, expected", len(bad), bad[:5], got[bad[:5]], want[bad[:5]]))
            assert not problems, problems
            line, _, storable, _, marked = ref.expected_lines(qw, L, bits)
            _, _, _, _, marked = ref.expected_lines(words, L, bits)  # (the marks are the table's, not the batch's)
            assert storable.all()
            in_marked = marked[line]
            absent = want == 0
            T = len(q2d)
            searched = absent & in_marked  # a miss that proves nothing
            assert searched.sum() > 1000 and (~in_marked).sum() > 1000
            assert int(census[6]) >= T + int(searched.sum()), (census, T, int(searched.sum()))
            # unmarked lines only, stored keys and misses alike: the table line and nothing else
            got, census = census_run(w.ix, q2d[~in_marked])
            assert np.array_equal(got, want[~in_marked])
            assert int(census[6]) == int((~in_marked).sum()), ("a query in an unmarked line costs its table line only", census, int((~in_marked).sum()))
            # misses in marked lines only: every one is searched behind its table line
            got, census = census_run(w.ix, q2d[searched])
            assert not got.any()
            assert int(census[6]) >= 2 * int(searched.sum()), ("a miss in a marked line must be searched", census, int(searched.sum()))
        finally:
            w.ix.set_kmer_table(0)


@pytest.mark.parametrize("L", [31, 32])
def test_tags_too_wide_for_the_line_bits(world, L):
    """(c) 2^12 lines: most tags do not fit beside 12 line bits, are not stored and mark their lines"""
    w = world
    words, counts = world_ref(w, L)
    rng = np.random.default_rng(300 + L)
    with forced_lines(1 << 12):
        try:
            tab, bits, info = fresh_table(w.ix, L, w.batch(L)[0])
            assert bits == 12
            _, _, storable, _, marked = ref.expected_lines(words, L, bits)
            assert (~storable).sum() > 100_000 and storable.sum() > 100
            entries, n_marked = ref.audit(tab, bits, L, words, counts)
            assert info["entries"] == entries and info["overflowed_lines"] == n_marked, (info, entries, n_marked)
            print("L = %d in 2^12 lines: %d of %d keys unstorable, %d entries, %d marked" % (L, int((~storable).sum()), len(words), entries, n_marked))
            # 20 000 present k-mers -- the stored ones all among them -- and 20 000 substituted ones
            keep = np.flatnonzero(storable)
            pick = np.concatenate([keep, rng.choice(len(words), size=20_000 - len(keep), replace=False)]) if len(keep) < 20_000 else keep[:20_000]
            pres = unpack(words[pick], L)
            near = substituted_head(pres, L - w.k, rng)
            q2d = np.concatenate([pres, near])
            want = lookup(words, counts, ref.pack_queries(q2d))
            assert (want[:len(pres)] > 0).all() and (want[len(pres):] == 0).mean() > 0.5
            got, _ = census_run(w.ix, q2d)
            bad = np.flatnonzero(got != want)
            assert len(bad) == 0, (len(bad), bad[:5], got[bad[:5]], want[bad[:5]])
            check_counts(w, L, False)  # and the oracle's batch
        finally:
            w.ix.set_kmer_table(0)


RUN = 1_048_595  # letters of the A run: A^20 occurs 2^20 times, A^21 KT_ASK times, A^22 KT_ASK - 1 times


def a_run_occurrences(text, L):
    """occurrences of A^L: the sum over the maximal runs of A of max(0, length - L + 1)"""
    is_a = np.concatenate([[False], text == ord("A"), [False]])
    edge = np.flatnonzero(is_a[1:] != is_a[:-1])
    lens = edge[1::2] - edge[0::2]
    return int(np.maximum(0, lens - L + 1).sum())


def test_count_field_saturation():
    """(d) a run of 1 048 595 A behind an N: A^20 occurs 2^20 times (above the field), A^21 exactly KT_ASK times (the value
    that doubles as "ask the index"), A^22 KT_ASK - 1 times (the largest count kept).  The N in front makes the run's first 32
    rows incomplete entries, so part of each count arrives one at a time on top of the run inserted in one piece.  Expected
    counts are run-length arithmetic and the text's own sliding windows.  (Windows across the run's left end hold the N and are
    no k-mers; their stand-ins are C..CA..A with the run's seed bucket, which the table must answer 0.  The oracle is left out:
    its prefix-doubling suffix sort takes far longer than a second on a homopolymer.)"""
    rng = np.random.default_rng(41)
    left, right = synth.NT[rng.integers(0, 4, size=100_000, dtype=np.uint8)], synth.NT[rng.integers(0, 4, size=100_000, dtype=np.uint8)]
    if right[0] == ord("A"):
        right[0] = ord("C")  # (the flank in front ends at the N: only this letter touches the run)
    text = np.concatenate([left, np.frombuffer(b"N", np.uint8), np.full(RUN, ord("A"), np.uint8), right, np.frombuffer(b"$", np.uint8)])
    run_end = len(left) + 1 + RUN  # the first letter behind the run
    assert a_run_occurrences(text, 20) == 1 << 20 and a_run_occurrences(text, 21) == ref.KT_ASK and a_run_occurrences(text, 22) == ref.KT_ASK - 1
    ix = FmIndex.from_text(text, 0, 8, 0, [0], ["one"]).set_devices([0])
    try:
        k = ix.seed_kmer_len()
        assert 8 <= k < 20 and ix.lcx_enabled() and ix.verify_enabled()
        batches = {}
        for L in (20, 21, 22):
            all_w, all_c = ref.kmer_counts(text, L)  # every L-mer of the text with its count
            assert int(lookup(all_w, all_c, np.zeros(1, np.uint64))[0]) == a_run_occurrences(text, L)
            qs = [np.full(L, ord("A"), np.uint8)]
            qs += [text[run_end - a:run_end - a + L] for a in range(1, L)]                                     # across the run's right end
            qs += [np.concatenate([np.full(L - a, ord(c), np.uint8), np.full(a, ord("A"), np.uint8)]) for a in range(k, L) for c in "CT"]
            q2d = np.concatenate([np.array(qs, dtype=np.uint8), synth.random_queries(1000, L, 0, L), synth.sampled_queries(text, 500, L, L),
                                  synth.sampled_queries(np.concatenate([left, right, text[-1:]]), 500, L, L + 1)])
            want = lookup(all_w, all_c, ref.pack_queries(q2d))
            assert want[0] == a_run_occurrences(text, L) and (want[1:L] >= 1).all()
            batches[L] = (q2d, want)
        for L, field, lines_of_a in ((20, ref.KT_ASK, None), (21, ref.KT_ASK, None), (22, ref.KT_ASK - 1, 1)):
            q2d, want = batches[L]
            ix.set_kmer_table(0)
            ix.set_kmer_table(1)
            got, _ = census_run(ix, q2d)
            bad = np.flatnonzero(got != want)
            assert len(bad) == 0, (L, len(bad), bad[:5], got[bad[:5]], want[bad[:5]])
            assert np.array_equal(ix.count_kmers_nt2(q2d, True), want), L
            tab, bits, info = read_table(ix, L)
            # A^L packs to 0 and kt_mix(0) = 0: line 0, tag 0
            slot = [int(e) for e in tab[:16] if int(e) & ref.KT_CNT_MASK and int(e) >> ref.KT_TAG_SHIFT == 0]
            assert len(slot) == 1 and slot[0] & ref.KT_CNT_MASK == field, (L, [hex(int(e)) for e in tab[:16]])
            got, census = census_run(ix, q2d[:1])
            assert int(got[0]) == int(want[0])
            print("L = %d: A^L occurs %d times, stored field %d, census[6] of A^L alone %d, table %r" % (L, int(want[0]), slot[0] & ref.KT_CNT_MASK, int(census[6]), info))
            if lines_of_a is None:
                assert int(census[6]) >= 2, ("a saturated entry asks the index", L, census)
            else:
                assert int(census[6]) == lines_of_a, ("the largest count the field keeps is answered by the table line", L, census)
            if L == 22:
                words, counts = ref.reference_table(text, k, L)
                assert len(words) >= 1 and counts.max() == ref.KT_ASK - 1
                entries, marked = ref.audit(tab, bits, L, words, counts)
                assert info["entries"] == entries and info["overflowed_lines"] == marked, (info, entries, marked)
        ix.set_kmer_table(0)
        for L in (20, 21, 22):
            q2d, want = batches[L]
            got, _ = census_run(ix, q2d)
            assert np.array_equal(got, want), L
            assert ix.kmer_table_info()["length"] == 0
    finally:
        ix.close()


def test_two_lengths_in_flight_from_two_host_threads(world):
    """(e) each launch of one thread replaces the table the other thread's launch, still running, was given: replacing takes
    the lock exclusively and freeing waits for the device, so no kernel runs on a freed table -- all eight outputs are the
    oracle's and whichever table is left audits clean"""
    import torch
    w = world
    order = {0: (21, 31, 21, 31), 1: (31, 21, 31, 21)}
    w.ix.set_kmer_table(0)
    w.ix.set_kmer_table(1)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    bufs, d_words, want, n = [], {}, {}, {}
    errors, spans, gate = [], [], threading.Barrier(2)
    try:
        for L in (21, 31):
            q2d, want[L], _, _ = w.batch(L)
            q2d = np.concatenate([q2d] * 4)  # (42 000 k-mers: a launch that lasts while the other thread gets going)
            want[L] = np.concatenate([want[L]] * 4)
            n[L] = len(q2d)
            d_ascii, d_bad = w.ix.dev_upload(np.ascontiguousarray(q2d).reshape(-1)), w.ix.dev_malloc(8)
            d_words[L] = w.ix.dev_malloc(8 * n[L])
            bufs += [d_ascii, d_bad, d_words[L]]
            w.ix.dev_memset(d_bad, 0, 8)
            w.ix.dev_pack_nt2(d_ascii, n[L], L, d_words[L], d_bad)
            w.ix.dev_synchronize()
            assert int(w.ix.dev_download(d_bad, (1,), np.uint64)[0]) == 0
        d_out = {}
        for i in (0, 1):
            for r, L in enumerate(order[i]):
                d_out[i, r] = w.ix.dev_malloc(8 * n[L])
                bufs.append(d_out[i, r])
                w.ix.dev_memset(d_out[i, r], 0xFF, 8 * n[L])
        w.ix.dev_synchronize()

        def run(i):
            try:
                torch.cuda.set_device(0)
                for r, L in enumerate(order[i]):
                    gate.wait(timeout=60)
                    t0 = time.perf_counter()
                    w.ix.dev_count_nt2(d_words[L], n[L], L, d_out[i, r], True, streams[i].cuda_stream)
                    t1 = time.perf_counter()
                    streams[i].synchronize()
                    spans.append((i, r, L, round(1e3 * (t1 - t0), 2), round(1e3 * (time.perf_counter() - t1), 2)))
            except BaseException as e:  # noqa: BLE001
                errors.append(repr(e))
                gate.abort()

        threads = [threading.Thread(target=run, args=(i,), daemon=True) for i in (0, 1)]
        for t in threads:
            t.start()
        for t in threads:
            t.join(timeout=60)
        assert not any(t.is_alive() for t in threads), "a thread is still running after 60 s"
        assert not errors, errors
        print("(thread, round, L, ms in the launch call, ms until its stream was idle):", sorted(spans))
        w.ix.dev_synchronize()
        for i in (0, 1):
            for r, L in enumerate(order[i]):
                got = w.ix.dev_download(d_out[i, r], (n[L],), np.uint64)
                bad = np.flatnonzero(got != want[L])
                assert len(bad) == 0, (i, r, L, len(bad), bad[:5], got[bad[:5]], want[L][bad[:5]])
        L = w.ix.kmer_table_info()["length"]
        assert L in (21, 31)
        audit_resident(w.ix, L, *world_ref(w, L))
    finally:
        w.ix.dev_synchronize()
        for p in bufs:
            w.ix.dev_free(p)
        w.ix.set_kmer_table(0)


def test_a_new_seed_length_drops_and_rebuilds_the_table(world):
    """(f) build_seed drops the table with the index it is made of; the next launch builds the table of the new k"""
    w, L = world, 21
    k = w.k
    fresh_table(w.ix, L, w.batch(L)[0])
    try:
        w.ix.set_seed_kmer_len(k - 1)
        assert w.ix.kmer_table_info()["length"] == 0 and w.ix.debug_kmer_table() is None
        assert w.ix.seed_kmer_len() == k - 1 and w.ix.lcx_enabled()
        check_counts(w, L, False)  # (builds the table of k - 1: mode 1 is still asked for)
        audit_resident(w.ix, L, *world_ref(w, L, k - 1))
    finally:
        w.ix.set_seed_kmer_len(k)
    assert w.ix.kmer_table_info()["length"] == 0 and w.ix.seed_kmer_len() == k and w.ix.lcx_enabled()
    w.ix.count_kmers_nt2(w.batch(L)[0][:100], True)
    audit_resident(w.ix, L, *world_ref(w, L))
    check_counts(w, L, False)
    w.ix.set_kmer_table(0)


def test_a_sparser_locate_sa_drops_the_table(world):
    """(f) build_dense_sa drops the table (it is built from the ratio-1 dense SA and the text); without them the generic schedule
    counts, and the table comes back with them"""
    w, L = world, 31
    q2d, want, _, _ = w.batch(L)
    fresh_table(w.ix, L, q2d)
    try:
        w.ix.set_locate_sa_ratio(2)
        assert w.ix.kmer_table_info()["length"] == 0 and w.ix.debug_kmer_table() is None
        assert "k-mer count table" not in w.ix.count_schedule(L), w.ix.count_schedule(L)
        assert np.array_equal(w.ix.count_kmers_nt2(q2d, True), want)
        assert np.array_equal(w.ix.parallel_count_csr(*synth.fixed_to_csr(q2d)), want)
        assert w.ix.kmer_table_info()["length"] == 0
    finally:
        w.ix.set_locate_sa_ratio(1)
        w.ix.set_verify(2)
        w.ix.set_lcx(True)
    assert w.ix.lcx_enabled() and w.ix.verify_enabled() and w.ix.seed_kmer_len() == w.k
    assert "k-mer count table" in w.ix.count_schedule(L)
    assert w.ix.kmer_table_info()["length"] == 0
    w.ix.count_kmers_nt2(q2d[:100], True)
    audit_resident(w.ix, L, *world_ref(w, L))
    check_counts(w, L, False)
    w.ix.set_kmer_table(0)


def test_a_rebuilt_replica_inherits_the_request_and_not_the_table(world):
    """(f) set_devices makes a new replica: it has no table, keeps awry_set_kmer_table(1), and builds on its first launch"""
    w, L = world, 21
    fresh_table(w.ix, L, w.batch(L)[0])
    w.ix.set_devices([0])
    assert w.ix.kmer_table_info()["length"] == 0 and w.ix.debug_kmer_table() is None
    assert w.ix.seed_kmer_len() == w.k and w.ix.lcx_enabled() and w.ix.verify_enabled()
    w.ix.count_kmers_nt2(w.batch(L)[0][:100], True)
    audit_resident(w.ix, L, *world_ref(w, L))
    check_counts(w, L, False)
    w.ix.set_kmer_table(0)


def test_host_batches_of_three_lengths(world):
    """(f) 30 000 queries of lengths 21, 25 and 31 through the host path.  Mixed in one call they are a ragged batch: that takes
    the reads kernels (launch_count_nt2_long with a length per query), which never consult the table -- the call neither builds
    one nor disturbs the one that is resident.  One call per length is a k-mer batch each: every call replaces the table with
    the one of its length."""
    w = world
    rng = np.random.default_rng(55)
    groups = {}
    for L in (21, 25, 31):
        pres = synth.sampled_queries(w.text, 7000, L, 60 + L)
        groups[L] = np.concatenate([pres, substituted_head(pres[:2000], L, rng), synth.random_queries(1000, L, 0, L)])
    qs = [bytes(q) for L in groups for q in groups[L]]
    qs = [qs[j] for j in rng.permutation(len(qs)).tolist()]
    assert len(qs) == 30_000
    from awry_amd.fm_index import pack_queries
    qb, qo = pack_queries(qs)
    want, _ = w.oi.parallel_count(qb, qo, 4)
    w.ix.set_kmer_table(0)
    w.ix.set_kmer_table(1)
    try:
        got = w.ix.parallel_count_csr(qb, qo)
        bad = np.flatnonzero(got != want)
        assert len(bad) == 0, (len(bad), bad[:5], got[bad[:5]], want[bad[:5]])
        assert w.ix.kmer_table_info()["length"] == 0, "a ragged batch takes the reads kernels: no table"
        for L in (21, 25, 31, 21):
            want_L, _ = w.oi.parallel_count(*synth.fixed_to_csr(groups[L]), 4)
            assert np.array_equal(w.ix.parallel_count_csr(*synth.fixed_to_csr(groups[L])), want_L), L
            audit_resident(w.ix, L, *world_ref(w, L))
        assert np.array_equal(w.ix.parallel_count_csr(qb, qo), want)
        audit_resident(w.ix, 21, *world_ref(w, 21))  # (the ragged call left the resident table alone)
    finally:
        w.ix.set_kmer_table(0)


def test_a_text_with_no_covered_bucket(oracle):
    """(f) 3 000 i.i.d. letters: no seed bucket has more than 4 rows, so the table is empty -- and still resident and consulted"""
    L = 21
    text, st, hd = synth.make_text(3000, 0, 77)
    ix = FmIndex.from_text(text, 0, 8, 0, st, hd).set_devices([0])
    oi = oracle.OracleIndex.from_text(text, 0, 8, 0, st, hd)
    try:
        k = ix.seed_kmer_len()
        assert 0 < k < L and int(ref.kmer_counts(text, k)[1].max()) <= ref.LANE_ROWS
        words, counts = ref.reference_table(text, k, L)
        assert len(words) == 0
        q2d = np.concatenate([synth.sampled_queries(text, 1000, L, 5), synth.random_queries(1000, L, 0, 6)])
        want, _ = oi.parallel_count(*synth.fixed_to_csr(q2d), 4)
        ix.set_kmer_table(1)
        got, _ = census_run(ix, q2d)
        assert np.array_equal(got, want)
        assert np.array_equal(ix.parallel_count_csr(*synth.fixed_to_csr(q2d)), want)
        info = ix.kmer_table_info()
        if not ix.lcx_enabled():
            assert info["length"] == 0, info
        else:
            assert info["length"] == L and info["entries"] == 0 and info["overflowed_lines"] == 0, info
            tab, bits, info = audit_resident(ix, L, words, counts)
            assert not tab.any()
            got, _ = census_run(ix, q2d)
            assert np.array_equal(got, want)
    finally:
        ix.close()
        oi.close()
