"""The benchmark's default workload at its full size against the oracle: the repeat-rich, GRCh38-shaped 3.1 Gbp text that
bench.py builds by default (workload_text: synth.repeat_rich_text with the same length, seed and records; ~43 % of it in
repeat families).  On this text most queries are decided by the left-context index or fall back to LF steps -- what the
i.i.d. full-scale tests hardly reach: multi-level node searches and bucket tails in lcx_quad_body, RS_LCX / RS_SINGLE
range starts and the locate order that follows from them, count_nt2_reads_pool_kernel.

One index for the module (a replica with every accelerator takes ~209 GB: two do not fit on one card).  One batch of
31-mers and 101-bp reads -- present, one substitution, random, and a heavy set the oracle counts at 2..8 and at more than 8
-- through five entry points in four configurations.  Counts of the whole batch are the oracle's; locations and their order
are the oracle's on a sample of at most ~2 M hits; configurations and entry points agree bit for bit on the whole batch."""
import os
import time

import numpy as np
import pytest

from awry_amd.fm_index import FmIndex
from tests import mismatch_ref as mr
from tests import synth

pytestmark = pytest.mark.gpu

N_TEXT, RECORDS, TEXT_SEED = 3_100_000_000, 25, 0xA5A50000 + 6  # bench.py: WORKLOADS["grch38-repeats"], workload_text()
ORACLE_HITS = 2_000_000  # the oracle's locate budget: satellite windows have 10^4 .. 10^5 hits each
THREADS = 16
MM_HIT_BUDGET = 1 << 24  # hits one mismatch locate call of the sample may return (a host-memory guard: 25 B per hit, not a tolerance)
MM_LIGHT = 4096          # sample queries with at most this many hits are all located; heavier ones while the budget lasts
# (length, present windows, uniform windows the heavy set is drawn from, most of them kept at 2..8 / at more than 8 hits, seed)
GROUPS = ((31, 100_000, 400_000, 20_000, 5_000, 31), (101, 50_000, 200_000, 10_000, 5_000, 101))


def substitute(q2d, rng):
    """one substitution per query, at a random column, to another letter"""
    out = q2d.copy()
    r, col = np.arange(len(out)), rng.integers(0, out.shape[1], size=len(out))
    out[r, col] = synth.NT[(np.searchsorted(synth.NT, out[r, col]) + rng.integers(1, 4, size=len(out))) % 4]
    return out


def make_group(text, oi, L, m, m_heavy, keep_mid, keep_hi, seed):
    """-> (queries uint8[., L], text position of each query drawn from the text or -1): m windows at uniform positions
    (windows with N excluded), m / 4 of them with one substitution, m / 4 random; then from m_heavy more windows the ones the
    oracle counts at 2..8 (RS_LCX) and at more than 8 (LF pool / RS_PLAIN), at most keep_mid / keep_hi of them"""
    rng = np.random.default_rng(seed)
    pos = rng.integers(0, len(text) - 1 - L, size=2 * (m + m_heavy))
    win = text[pos[:, None] + np.arange(L)[None, :]]
    ok = ~(win == ord("N")).any(axis=1)
    pos, win = pos[ok], win[ok]
    assert len(pos) >= m + m_heavy
    c, _ = oi.parallel_count(*synth.fixed_to_csr(win[m:m + m_heavy]), THREADS)
    hp, hw = pos[m:m + m_heavy], win[m:m + m_heavy]
    mid, hi = np.flatnonzero((c >= 2) & (c <= 8))[:keep_mid], np.flatnonzero(c > 8)[:keep_hi]
    assert len(mid) >= 1000 and len(hi) >= 500, (L, len(mid), len(hi))
    q = np.concatenate([win[:m], substitute(win[:m // 4], rng), synth.random_queries(m // 4, L, 0, seed + 1), hw[mid], hw[hi]])
    p = np.concatenate([pos[:m], np.full(m // 2, -1), hp[mid], hp[hi]])
    return q, p


def segments(off, sel, *arrays):
    """the CSR rows `sel` of a locate result: (offsets of the selection, each array's entries of those rows in that order)"""
    lens = np.diff(off).astype(np.int64)[sel]
    o = np.zeros(len(sel) + 1, dtype=np.uint64)
    o[1:] = np.cumsum(lens)
    src = np.repeat(off[:-1][sel].astype(np.int64) - o[:-1].astype(np.int64), lens) + np.arange(int(o[-1]))
    return (o,) + tuple(a[src] for a in arrays)


def count_with_census(ix, q2d):
    """counts and the 8-word census of awry_dev_count_nt2_tally (word 6: left-context index nodes)"""
    n, L = q2d.shape
    d_ascii = ix.dev_upload(np.ascontiguousarray(q2d).reshape(-1))
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


def run_batch(ix, b):
    """every entry point on the batch -> dict of results, all in CSR order except the per-group ones"""
    out = {"count_batch": ix.parallel_count_csr(b["qb"], b["qo"])}
    d_q, d_o = ix.dev_upload(b["qb"]), ix.dev_upload(b["qo"])
    d_c = ix.dev_malloc(8 * b["n"])
    try:
        ix.dev_count_ascii(d_q, d_o, b["n"], d_c)
        ix.dev_synchronize()
        out["dev_count_ascii"] = ix.dev_download(d_c, (b["n"],), np.uint64)
    finally:
        for p in (d_q, d_o, d_c):
            ix.dev_free(p)
    out["count_kmers_nt2"], out["census"] = count_with_census(ix, b["groups"][0][0])
    out["locate_batch"] = ix.parallel_locate_csr(b["qb"], b["qo"])
    out["locate_reads_nt2"] = [ix.locate_reads_nt2(q) for q, _, _ in b["groups"]]
    return out


def mismatch_sample(text, oi, q31_group):
    """the substitution-tolerant legs' sample, with the oracle's variant-enumeration counts (mismatch_ref.oracle_counts_batch)
    while its index is open: ~1 500 31-mers (present, 1 and 2 planted substitutions, random, and the exact path's heavy set:
    windows of the repeat families, which meet their diverged copies), 500 16-mers (at 3.1 Gbp most of a 16-mer's 1 985
    variants at k = 2 occur) and 300 101-bp reads (k = 1 on all, k = 2 on 50).
    -> [(name, queries uint8[., L], k, counts uint64[., k + 1], rows to locate, [(row, oracle_locate result)])]"""
    t0 = time.time()
    rng = np.random.default_rng(77)
    s31 = synth.sampled_queries(text, 1000, 31, 771)
    q31 = np.concatenate([s31[:400], substitute(s31[400:700], rng), substitute(substitute(s31[700:], rng), rng),
                          synth.random_queries(300, 31, 0, 772), q31_group[-200:]])
    s16 = synth.sampled_queries(text, 250, 16, 773)
    q16 = np.concatenate([s16, synth.random_queries(250, 16, 0, 774)])
    s101 = synth.sampled_queries(text, 300, 101, 775)
    reads = np.concatenate([s101[:100], substitute(s101[100:200], rng), substitute(substitute(s101[200:], rng), rng)])
    reads = reads[rng.permutation(len(reads))]
    legs = []
    for name, q, k, n_order in (("31-mers", q31, 2, 24), ("16-mers", q16, 2, 24), ("reads", reads, 1, 8), ("reads", reads[:50], 2, 4)):
        counts, _ = mr.oracle_counts_batch(oi, [bytes(r) for r in q], k, 0, THREADS)
        ks = (1, 2) if k == 2 and name != "reads" else (k,)
        for kk in ks:
            tot = counts[:, :kk + 1].sum(axis=1).astype(np.int64)
            rows, n_heavy = mr.budgeted_rows(tot, MM_LIGHT, MM_HIT_BUDGET, 780 + kk)
            cand = np.flatnonzero((tot >= 1) & (tot <= 3000))
            pick = np.random.default_rng(790 + kk).choice(cand, size=min(n_order, len(cand)), replace=False)
            order = [(int(i), mr.oracle_locate(oi, bytes(q[i]), kk, 0)) for i in np.sort(pick)]
            legs.append((name, q, kk, counts[:, :kk + 1], rows, n_heavy, order))
    return legs, time.time() - t0


@pytest.fixture(scope="module")
def repeats(oracle, tmp_path_factory):
    import torch
    t0 = time.time()
    text, st, hd, _ = synth.repeat_rich_text(N_TEXT, TEXT_SEED, RECORDS, device="cuda:0")
    torch.cuda.empty_cache()  # (the library sizes its accelerators from the HBM that is free)
    ix = FmIndex.from_text(text, 0, 8, 0, st, hd, build_device=0).set_devices([0])
    try:
        assert ix.lcx_enabled() and ix.verify_enabled()
        path = str(tmp_path_factory.mktemp("repeats") / "r.awry")
        ix.save(path)
        oi = oracle.OracleIndex.load(path)
        os.remove(path)
        try:
            groups = []
            for spec in GROUPS:
                q, p = make_group(text, oi, *spec)
                groups.append([q, p, None])
            # one CSR batch of all queries in a random order (the host entry points pack it as ragged reads, chunk by chunk)
            lens = np.concatenate([np.full(len(q), q.shape[1], np.int64) for q, _, _ in groups])
            flat = np.concatenate([q.reshape(-1) for q, _, _ in groups])
            starts = np.concatenate([[0], np.cumsum(lens)[:-1]])
            perm = np.random.default_rng(5).permutation(len(lens))
            qo = np.zeros(len(lens) + 1, dtype=np.uint64)
            qo[1:] = np.cumsum(lens[perm])
            qb = flat[np.repeat(starts[perm], lens[perm]) + np.arange(int(qo[-1])) - np.repeat(qo[:-1].astype(np.int64), lens[perm])]
            inv = np.empty(len(perm), dtype=np.int64)
            inv[perm] = np.arange(len(perm))
            base = 0
            for g in groups:
                g[2] = inv[base:base + len(g[0])]  # CSR rows of the group's queries, in the group's order
                base += len(g[0])
            b = {"qb": qb, "qo": qo, "n": len(lens), "groups": groups, "lens": lens[perm]}
            want, _ = oi.parallel_count(qb, qo, THREADS)
            # the locate sample: every query with at most 8 hits, then heavier ones in a random order while the budget lasts
            light = np.flatnonzero(want <= 8)
            budget = ORACLE_HITS - int(want[light].sum())
            assert budget > ORACLE_HITS // 4
            heavy = []
            for i in np.random.default_rng(6).permutation(np.flatnonzero(want > 8)).tolist():
                if int(want[i]) <= budget:
                    heavy.append(i)
                    budget -= int(want[i])
            sample = np.sort(np.concatenate([light, np.array(heavy, dtype=np.int64)]))
            so = np.zeros(len(sample) + 1, dtype=np.uint64)
            so[1:] = np.cumsum(b["lens"][sample])
            sb = qb[np.repeat(qo[:-1][sample].astype(np.int64) - so[:-1].astype(np.int64), b["lens"][sample]) + np.arange(int(so[-1]))]
            ooff, ogpos, opos, _ = oi.parallel_locate(sb, so, THREADS)
            t_mm = time.time()
            mm_legs, mm_ref_s = mismatch_sample(text, oi, groups[0][0])
        finally:
            oi.close()
        t0 += time.time() - t_mm  # (setup_s below stays the exact legs' setup; the mismatch sample reports its own time)
        b.update(mm_legs=mm_legs, mm_ref_s=mm_ref_s)
        b.update(text=text, starts=np.array(st, dtype=np.uint64), want=want, sample=sample, oracle_loc=(ooff, ogpos, opos),
                 n_heavy=len(heavy), setup_s=time.time() - t0)
        yield ix, b
    finally:
        ix.close()


def test_defaults_match_the_oracle(repeats):
    ix, b = repeats
    t0 = time.time()
    text, want = b["text"], b["want"]
    r = run_batch(ix, b)
    b["ref"] = r
    counts = r["count_batch"]
    bad = np.flatnonzero(counts != want)
    assert len(bad) == 0, (len(bad), bad[:5], counts[bad[:5]], want[bad[:5]])
    assert np.array_equal(r["dev_count_ascii"], want)
    q31, _, rows31 = b["groups"][0]
    assert np.array_equal(r["count_kmers_nt2"], want[rows31])
    assert int(r["census"][6]) > 0, ("the left-context index should decide k-mers here", r["census"])
    # the classes the batch is built to reach
    assert int(((want >= 2) & (want <= 8)).sum()) >= 2000 and int((want > 8).sum()) >= 1000 and int(want.max()) >= 5_000
    off, g, p = r["locate_batch"]
    assert np.array_equal(np.diff(off), counts)
    # the oracle's locations, in the oracle's order, on the sample
    ooff, ogpos, opos = b["oracle_loc"]
    so, sg, sp = segments(off, b["sample"], g, p)
    assert np.array_equal(so, ooff)
    assert np.array_equal(sg, ogpos)
    assert np.array_equal(sp, opos)
    assert b["n_heavy"] >= 100, "the locate sample should hold queries with more than 8 hits"
    # every located window is its query, every query drawn from the text is found at its own position, (record, offset)
    for q, pos, rows in b["groups"]:
        L = q.shape[1]
        go, gg = segments(off, rows, g)
        qi = np.repeat(np.arange(len(rows)), np.diff(go).astype(np.int64))
        for a in range(0, len(gg), 1 << 22):
            e = min(len(gg), a + (1 << 22))
            assert np.array_equal(text[gg[a:e].astype(np.int64)[:, None] + np.arange(L)[None, :]], q[qi[a:e]]), L
        found = np.zeros(len(rows), dtype=bool)
        found[qi[gg.astype(np.int64) == pos[qi]]] = True
        assert found[pos >= 0].all(), L
    si = np.searchsorted(b["starts"], g, side="right") - 1
    assert np.array_equal(p[:, 0], si.astype(np.uint64)) and np.array_equal(p[:, 1], g - b["starts"][si])
    # the packed device pipeline: the CSR rows of each group, in the group's order
    for (q, _, rows), (o2, g2, p2) in zip(b["groups"], r["locate_reads_nt2"]):
        so, sg, sp = segments(off, rows, g, p)
        assert np.array_equal(o2, so) and np.array_equal(g2, sg) and np.array_equal(p2, sp), q.shape[1]
    hist = np.bincount(text, minlength=256)
    ps = ix.prefix_sums()
    assert [int(ps[i + 1] - ps[i]) for i in range(6)] == [1, hist[65], hist[67], hist[71], hist[78], hist[84]]
    print("repeat-rich full scale: setup %.1f s, defaults %.1f s, %d queries, %d hits, locate sample %d queries (%d heavy), %d oracle hits"
          % (b["setup_s"], time.time() - t0, b["n"], int(off[-1]), len(b["sample"]), b["n_heavy"], len(ogpos)))


def test_configurations_agree(repeats):
    """the index off, on again, and seed-and-verify off with locate walking to the file's samples: the same results, bit for
    bit, from every entry point"""
    ix, b = repeats
    if "ref" not in b:
        pytest.fail("test_defaults_match_the_oracle did not leave its results")
    ref = b["ref"]

    def same(r, what):
        for k in ("count_batch", "dev_count_ascii", "count_kmers_nt2"):
            assert np.array_equal(r[k], ref[k]), (what, k)
        for x, y in zip(r["locate_batch"], ref["locate_batch"]):
            assert np.array_equal(x, y), (what, "locate_batch")
        for a, c in zip(r["locate_reads_nt2"], ref["locate_reads_nt2"]):
            for x, y in zip(a, c):
                assert np.array_equal(x, y), (what, "locate_reads_nt2")

    t0 = time.time()
    ix.set_lcx(False)
    assert not ix.lcx_enabled()
    r = run_batch(ix, b)
    same(r, "lcx off")
    assert int(r["census"][6]) == 0, r["census"]
    ix.set_lcx(True)
    assert ix.lcx_enabled()
    r = run_batch(ix, b)
    same(r, "lcx on again")
    assert int(r["census"][6]) > 0, r["census"]
    ix.set_verify(-1)
    ix.set_locate_sa_ratio(0)
    assert not ix.verify_enabled() and ix.locate_sa_ratio() == ix.suffix_array_compression_ratio()  # (no dense SA: the file's)
    same(run_batch(ix, b), "verify off, ratio 0")
    print("repeat-rich full scale: three more configurations %.1f s" % (time.time() - t0))


def test_mismatch_legs_match_the_oracle(repeats):
    """substitution-tolerant count and locate on the full-size index (rows beyond 2^31, the dense-SA / seed-and-verify
    locate fed from leaf lists): counts are the oracle's over all variants; the located hits are checked against the text
    itself (as many per query and distance as counted, distinct, every window free of '$' and at the reported distance),
    which is set equality with the definition; order and (record, offset) are mismatch_ref.oracle_locate's on a few dozen.
    Then 10^6 device-resident sampled 31-mers: column 0 at k = 2 is the exact count (which this module proves against the
    oracle), and columns 0..1 at k = 1 are columns 0..1 at k = 2."""
    ix, b = repeats
    t0 = time.time()
    text, starts = b["text"], b["starts"]
    report = []
    for name, q, k, want, rows, n_heavy, order in b["mm_legs"]:
        qb, qo = synth.fixed_to_csr(q)
        got = ix.parallel_count_mismatch_csr(qb, qo, k)
        bad = np.flatnonzero((got != want).any(axis=1))
        assert len(bad) == 0, (name, k, len(bad), bad[:5], got[bad[:5]], want[bad[:5]])
        sb, so = synth.fixed_to_csr(q[rows])
        off, g, p, d = ix.parallel_locate_mismatch_csr(sb, so, k)
        mr.assert_hits_are_the_definition(text, 0, q[rows], k, want[rows], off, g, d)
        si = np.searchsorted(starts, g, side="right") - 1
        assert np.array_equal(p[:, 0], si.astype(np.uint64)) and np.array_equal(p[:, 1], g - starts[si]), (name, k)
        at = {int(r): j for j, r in enumerate(rows)}
        for i, (og, op, od) in order:
            a, e = int(off[at[i]]), int(off[at[i] + 1])
            assert np.array_equal(g[a:e], og) and np.array_equal(p[a:e], op) and np.array_equal(d[a:e], od), (name, k, i)
        report.append("%s k = %d: %d counted, %d located (%d heavy), %d hits, order on %d" % (name, k, len(q), len(rows), n_heavy, len(g), len(order)))
    legs = {(name, k): (want, n_heavy) for name, q, k, want, rows, n_heavy, order in b["mm_legs"]}
    assert len(b["mm_legs"][0][1]) >= 1500 and legs[("31-mers", 2)][1] >= 10, "the 31-mer sample should hold located queries with thousands of hits"
    assert float(np.median(legs[("16-mers", 2)][0].sum(axis=1))) > 500
    # consistency on a device-resident batch
    n = 1_000_000
    q2d = synth.sampled_queries(text, n, 31, 799)
    qb, qo = synth.fixed_to_csr(q2d)
    d_q, d_o = ix.dev_upload(np.concatenate([qb, np.zeros(16, np.uint8)])), ix.dev_upload(qo)
    d_c, d_e = ix.dev_malloc(8 * n * 3), ix.dev_malloc(8 * n)
    try:
        ix.dev_count_ascii(d_q, d_o, n, d_e)
        ix.dev_count_mismatch(d_q, d_o, n, 2, d_c)
        ix.dev_synchronize()
        exact, c2 = ix.dev_download(d_e, (n,), np.uint64), ix.dev_download(d_c, (n, 3), np.uint64)
        ix.dev_count_mismatch(d_q, d_o, n, 1, d_c)
        ix.dev_synchronize()
        c1 = ix.dev_download(d_c, (n, 2), np.uint64)
    finally:
        for ptr in (d_q, d_o, d_c, d_e):
            ix.dev_free(ptr)
    assert (exact >= 1).all() and np.array_equal(c2[:, 0], exact) and np.array_equal(c1, c2[:, :2])
    print("repeat-rich full scale, mismatch legs: reference %.1f s, GPU legs and text checks %.1f s; %s; 10^6 resident 31-mers: %d hits at k = 2"
          % (b["mm_ref_s"], time.time() - t0, "; ".join(report), int(c2.sum())))
