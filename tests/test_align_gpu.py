"""The alignment of edit-distance hits on the GPU (awry_amd/csrc/kernels_align.hip.h, edit_host.h) against the definition in
tests/align_ref.py over the full table: text spans, CIGAR runs and offsets for exact equality, next to the arrays
awry_locate_edit_batch returns, which must come back byte-identical.  Reads are planted as tests/test_edit_gpu.py plants them.
Results must not depend on the accelerators, the seed table, the chunk capacity, the alignment sub-batch or the number of
replicas."""
import os
import subprocess

import numpy as np
import pytest

import awry_amd
from awry_amd import cigar_string
from awry_amd.fm_index import ALIGN_MAX_OPS, Q_CANDIDATE_CAP, FmIndex, pack_queries
from tests import align_ref as al
from tests import edit_ref as er
from tests import synth
from tests import test_edit_gpu as eg

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_CAP = eg.NO_CAP
LENGTHS = (20, 63, 64, 65, 101, 255, 256)


def same(a, b):
    return len(a) == len(b) and all(x.dtype == y.dtype and np.array_equal(x, y) for x, y in zip(a, b))


def check(w, qs, k, ix=None, max_candidates=NO_CAP):
    """one batch call against the reference; -> the library's arrays"""
    ix = w.ix if ix is None else ix
    got = ix.parallel_align_edit_csr(*pack_queries(qs), k, max_candidates)
    off, g, p, d, st, tl, coff, cg = got
    woff, wg, wd, wst, wtl, wcoff, wcg = al.align(w.t, qs, k, max_candidates)
    assert st.dtype == np.uint8 and np.array_equal(st, wst)
    if max_candidates == NO_CAP:
        assert not st.any()
    assert np.array_equal(off, woff) and np.array_equal(g, wg) and np.array_equal(d, wd), (k, [len(q) for q in qs])
    rec = np.searchsorted(w.st, g, side="right") - 1
    assert np.array_equal(p[:, 0], rec.astype(np.uint64)) and np.array_equal(p[:, 1], g - w.st[rec])
    assert tl.dtype == np.uint32 and coff.dtype == np.uint64 and cg.dtype == np.uint32
    assert np.array_equal(tl, wtl), (k, np.nonzero(tl != wtl)[0][:5])
    assert np.array_equal(coff, wcoff)
    assert np.array_equal(cg, wcg)
    assert int(np.diff(coff.astype(np.int64)).max(initial=0)) <= 2 * k + 1 <= ALIGN_MAX_OPS
    return got


def cigars(got, i):
    """the CIGAR strings of query i's hits"""
    off, coff, cg = got[0], got[6], got[7]
    return [cigar_string(cg[coff[h]:coff[h + 1]]) for h in range(int(off[i]), int(off[i + 1]))]


@pytest.fixture(scope="module")
def nt():
    return eg.World(*synth.make_text(20_000, 0, 51, 5, 0.01), 0)


@pytest.mark.parametrize("k", [0, 1, 3, 8])
def test_planted_edits_at_the_band_and_word_edges(nt, k):
    rng = np.random.default_rng(200 + k)
    qs = []
    for L in sorted(set((k + 1, 2 * (k + 1)) + LENGTHS)):
        reads = eg.reads_for(nt, rng, L, k)[0]
        qs += reads if L > 20 or k < 8 else reads[:2] + reads[-2:]  # (a 9-mer within 8 edits hits everywhere: four reads do)
    got = check(nt, qs, k)
    assert len(got[1]) > 60
    if k == 0:
        for i, q in enumerate(qs):
            assert set(cigars(got, i)) <= {"%d=" % len(q)}
    else:
        ops = set("".join(cigar_string(got[7])))
        assert {"=", "X", "I", "D"} <= ops


@pytest.mark.parametrize("k", [2, 4, 5, 6, 7])
def test_every_band_half_width(nt, k):
    """the launch's half-width is the smallest of 2, 4, 6, 8 that holds k: the widths and the distances just below them"""
    rng = np.random.default_rng(290 + k)
    qs = []
    for L in (33, 101, 130):
        qs += eg.reads_for(nt, rng, L, k)[0]
    got = check(nt, qs, k)
    assert int(got[3].max()) == k and len(got[1]) >= len(qs) - 4


@pytest.fixture(scope="module")
def runs():
    """the text of tests/test_edit_gpu.py's tandem arrays: a homopolymer and arrays of period 2 and 3 between random flanks"""
    rng = np.random.default_rng(52)
    rnd = lambda m: bytes(synth.NT[rng.integers(0, 4, size=m)])
    body = rnd(300) + b"A" * 200 + b"CT" + b"AC" * 120 + b"GG" + b"ACG" * 90 + rnd(300) + b"T" * 90
    text = np.frombuffer(body + b"$", np.uint8).copy()
    return eg.World(text, [0], ["r0"], 0)


@pytest.mark.parametrize("k", [1, 3])
def test_ties_in_homopolymers_and_tandem_arrays(runs, k):
    t = runs.text
    qs = [b"A" * 30, b"A" * 35 + b"C" + b"A" * 34, b"AC" * 20, b"AC" * 10 + b"A" + b"AC" * 10, b"ACG" * 15, b"ACG" * 7 + b"AG" + b"ACG" * 7,
          bytes(t[280:300]) + b"A" * 201 + bytes(t[500:520]),            # a flanked homopolymer one longer in the read: the 'I' goes left
          bytes(t[280:300]) + b"A" * 199 + bytes(t[500:520]),            # ... one shorter: the 'D'
          bytes(t[490:502]) + b"AC" * 40 + b"AAC" + b"AC" * 40,         # an insertion inside the period-2 array, anchored on its left flank
          b"AC" * 50 + b"C" + b"AC" * 50 + bytes(t[742:754]),            # a deletion inside it, anchored on its right flank
          bytes(t[742:744]) + b"ACG" * 30 + b"ACGG" + b"ACG" * 30,       # an insertion inside the period-3 array
          b"GT" + b"A" * 63, b"T" * 64]
    got = check(runs, qs, k)
    assert "20=1I220=" in cigars(got, 6) and "20=1D219=" in cigars(got, 7)
    assert len(got[1]) > 200  # plateaus are aligned whole


@pytest.mark.parametrize("k", [2, 3])
def test_text_ends_and_overhanging_reads(nt, k):
    rng = np.random.default_rng(210 + k)
    rnd = lambda m: bytes(synth.NT[rng.integers(0, 4, size=m)])
    n, text = nt.n, nt.text
    over = bytes([eg.other(nt.letters, text[n - 1])])  # (a letter that differs from the text's last: the 'I's cannot move left)
    qs = [bytes(text[:40]), bytes(text[1:41]), rnd(2) + bytes(text[:40]), rnd(k) + bytes(text[:64]),
          bytes(text[n - 40:n]), bytes(text[n - 41:n - 1]), bytes(text[n - 40:n]) + over * 2, bytes(text[n - 64:n]) + over * k,
          bytes(text[n - 3:n]) + b"A", bytes(text[:k + 1])]
    got = check(nt, qs, k)
    off, g, tl = got[0], got[1], got[5]
    assert g[off[0]] == 0 and cigars(got, 0)[0] == "40="                          # a hit at start 0
    assert cigars(got, 2)[0] == "2I40="                                            # a read hanging over the text's start
    assert int(g[off[5] - 1]) == n - 40 and int(tl[off[5] - 1]) == 40               # a hit in the last L symbols, ending at n
    h = int(off[7] - 1)                                                            # a read hanging over the text's end:
    assert int(g[h]) == n - 40 and int(tl[h]) == 40 and cigars(got, 6)[-1] == "40=2I"   # J = n - s cuts the table; the script ends in 'I's
    h = int(off[8] - 1)
    assert int(g[h]) + int(tl[h]) == n and cigars(got, 7)[-1] == "64=%dI" % k


@pytest.mark.parametrize("k", [1, 3])
def test_record_joins_and_n_runs(nt, k):
    text = nt.text
    joins = [int(s) - 1 for s in nt.st[1:]]
    assert all(text[j] == ord("N") for j in joins)
    nruns = np.nonzero((text[:-1] == ord("N")) & (np.roll(text[:-1], 1) == ord("N")))[0]
    r0 = int(nruns[0]) - 1  # the first letter of an N run
    qs = []
    for j in joins[:3]:
        q = bytes(text[j - 30:j + 31])
        qs += [q, q.replace(b"N", b"A"), q.replace(b"N", b"")]  # N in the read; a letter there; the join left out
    for a, b in ((r0 - 40, r0 + 3), (r0 - 40, r0 + 12), (r0 - 20, r0 + 1)):
        q = bytes(text[a:b])
        qs += [q, q.replace(b"N", b"C")]
    got = check(nt, qs, k)
    assert "61=" in cigars(got, 0)          # query N on text N is '='
    assert "30=1X30=" in cigars(got, 1)     # a letter on the join's N: 'X'
    assert "30=1D30=" in cigars(got, 2)     # the join left out of the read: 'D' covers the N


@pytest.fixture(scope="module")
def aa():
    return eg.World(*synth.make_text(5_000, 1, 53, 3, 0.01), 1)


@pytest.mark.parametrize("k", [1, 3])
def test_amino_with_x_in_text_and_query(aa, k):
    rng = np.random.default_rng(230 + k)
    qs = []
    for L in (12, 64, 65, 130):
        qs += eg.reads_for(aa, rng, L, k)[0]
    xs = np.nonzero(aa.text[:-1] == ord("X"))[0]
    xs = xs[(xs > 40) & (xs < aa.n - 40)]
    assert len(xs) >= 2
    for x in xs[:2]:
        q = bytes(aa.text[int(x) - 20:int(x) + 21])
        assert b"X" in q
        qs += [q, q.replace(b"X", b"A"), q[:10] + b"X" + q[11:]]  # X on X; a letter on the text's X; X on a text letter
    got = check(aa, qs, k)
    assert len(got[1]) >= 12 and "41=" in cigars(got, len(qs) - 3)


@pytest.fixture(scope="module")
def family():
    """tests/test_edit_gpu.py's family: 10 k random letters, then 3 000 copies of a 12-letter unit, each followed by 4 random letters"""
    rng = np.random.default_rng(54)
    rnd = lambda m: synth.NT[rng.integers(0, 4, size=m)]
    unit = np.frombuffer(b"GATTACAGGCTC", np.uint8)
    copies = np.concatenate([np.concatenate([unit, rnd(4)]) for _ in range(3000)])
    text = np.concatenate([rnd(10_000), copies, np.frombuffer(b"$", np.uint8)])
    return eg.World(text, [0], ["r0"], 0)


def test_identity_with_locate_and_abandoned_queries(nt, family):
    rng = np.random.default_rng(240)
    qs = []
    for L in (20, 64, 101, 129):
        qs += eg.reads_for(nt, rng, L, 2)[0]
    qb, qo = pack_queries(qs)
    loc = nt.ix.parallel_locate_edit_csr(qb, qo, 2, NO_CAP)
    got = nt.ix.parallel_align_edit_csr(qb, qo, 2, NO_CAP)
    assert same(got[:5], loc) and all(x.tobytes() == y.tobytes() for x, y in zip(got[:5], loc))
    w = family
    qs = []
    for i in range(6):
        p = 10_000 + 16 * int(rng.integers(0, 2990))
        qs.append(bytes(w.text[p:p + 24]))                   # piece 0 is the unit: 3 000 occurrences
        qs.append(bytes(w.text[100 * i:100 * i + 24]))      # anywhere
    qb, qo = pack_queries(qs)
    loc = w.ix.parallel_locate_edit_csr(qb, qo, 1, 1000)
    got = check(w, qs, 1, max_candidates=1000)
    assert same(got[:5], loc)
    off, st, coff = got[0], got[4], got[6]
    assert sum(int(s) == Q_CANDIDATE_CAP for s in st) >= 6 and sum(int(s) == 0 for s in st) >= 6
    for i, s in enumerate(st):  # abandoned: no hits and no runs; their neighbours: untouched
        assert (off[i + 1] == off[i] and coff[off[i + 1]] == coff[off[i]]) if s else (off[i + 1] > off[i] and coff[off[i + 1]] > coff[off[i]])
    # the nullable outputs: text_len alone, the CIGAR alone
    import ctypes as C
    L_ = awry_amd.load_library()
    u64p, u32p = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)
    o1, tl = u64p(), u32p()
    assert L_.awry_align_edit_batch(w.ix._h, qb.ctypes.data, qo.ctypes.data_as(u64p), len(qs), 1, 1000, C.byref(o1), None, None, None, None, C.byref(tl),
                                    None, None) == 0
    tot = int(off[-1])
    assert np.array_equal(np.ctypeslib.as_array(tl, (tot,)), got[5]) and np.array_equal(np.ctypeslib.as_array(o1, (len(qs) + 1,)), off)
    o2, co, cg = u64p(), u64p(), u32p()
    assert L_.awry_align_edit_batch(w.ix._h, qb.ctypes.data, qo.ctypes.data_as(u64p), len(qs), 1, 1000, C.byref(o2), None, None, None, None, None,
                                    C.byref(co), C.byref(cg)) == 0
    assert np.array_equal(np.ctypeslib.as_array(co, (tot + 1,)), coff) and np.array_equal(np.ctypeslib.as_array(cg, (int(coff[-1]),)), got[7])
    for p in (o1, tl, o2, co, cg):
        L_.awry_free_buffer(p)


def test_results_do_not_depend_on_accelerators_chunks_sub_batches_or_replicas(nt):
    rng = np.random.default_rng(250)
    qs = []
    for L in (20, 64, 101, 129):
        qs += eg.reads_for(nt, rng, L, 2)[0]
    qb, qo = pack_queries(qs)
    ix = nt.ix
    run = lambda x=ix: x.parallel_align_edit_csr(qb, qo, 2, NO_CAP)
    base = check(nt, qs, 2)
    ix.set_verify(-1)  # the private copy of the text
    try:
        assert not ix.verify_enabled() and same(run(), base)
    finally:
        ix.set_verify(2)
    assert ix.verify_enabled() and same(run(), base)
    ix.set_lcx(False)
    try:
        assert same(run(), base)
    finally:
        ix.set_lcx(True)
    ix.set_seed_kmer_len(0)
    try:
        assert ix.seed_kmer_len() == 0 and same(run(), base)
    finally:
        ix.set_seed_kmer_len(-1)
    os.environ["AWRY_EDIT_CANDIDATE_CAP"] = "20"  # the chunk splits in halves, down to single queries
    try:
        assert same(run(), base)
    finally:
        del os.environ["AWRY_EDIT_CANDIDATE_CAP"]
    two = FmIndex.from_text(nt.text, 0, 8, 0, [int(s) for s in nt.st], ["seq%d" % i for i in range(len(nt.st))]).set_devices([0, 0])
    try:
        assert same(run(two), base)
    finally:
        two.close()


def test_sub_batches(nt):
    rng = np.random.default_rng(260)
    qs = []
    for L in (20, 65, 101):
        qs += eg.reads_for(nt, rng, L, 3)[0]
    base = check(nt, qs, 3)
    total = len(base[1])
    assert total > 40
    for sub in (1, 7, total - 1, total, total + 1):  # the boundary inside a chunk, at its end, and beyond it
        os.environ["AWRY_ALIGN_SUB_BATCH"] = str(sub)
        try:
            assert same(nt.ix.parallel_align_edit_csr(*pack_queries(qs), 3, NO_CAP), base), sub
        finally:
            del os.environ["AWRY_ALIGN_SUB_BATCH"]


def dev_align(w, qs, triples, k, tally=False):
    """dev_edit_align on hand-made triples [(query, start, distance)] -> (text_len[m], n_ops[m], ops[m, ALIGN_MAX_OPS], tally or None)"""
    ix = w.ix
    qb, qo = pack_queries(qs)
    m = len(triples)
    pad = np.concatenate([qb, np.zeros(16, np.uint8)])
    ptrs = [ix.dev_upload(a) for a in (pad, qo, np.array([x[0] for x in triples], np.uint32), np.array([x[1] for x in triples], np.uint64),
                                       np.array([x[2] for x in triples], np.uint8))]
    d_tl, d_n, d_ops, d_t = ix.dev_malloc(4 * m), ix.dev_malloc(m), ix.dev_malloc(4 * m * ALIGN_MAX_OPS), ix.dev_malloc(16)
    ix.dev_memset(d_t, 0, 16)
    ix.dev_memset(d_n, 0xEE, m)
    if tally:
        ix.dev_edit_align_tally(*ptrs, m, k, d_tl, d_n, d_ops, d_t)
    else:
        ix.dev_edit_align(*ptrs, m, k, d_tl, d_n, d_ops)
    ix.dev_synchronize()
    tl = ix.dev_download(d_tl, (m,), np.uint32)
    n_ops = ix.dev_download(d_n, (m,), np.uint8)
    ops = ix.dev_download(d_ops, (m * ALIGN_MAX_OPS,), np.uint32).reshape(m, ALIGN_MAX_OPS)
    t = ix.dev_download(d_t, (2,), np.uint64) if tally else None
    for p in ptrs + [d_tl, d_n, d_ops, d_t]:
        ix.dev_free(p)
    return tl, n_ops, ops, t


def test_device_entry_point_on_hand_made_triples(nt):
    rng = np.random.default_rng(270)
    k, n = 3, nt.n
    q0, _ = eg.planted(nt, rng, 101, [("s", 30), ("d", 70)], p=5000)
    q1 = bytes(nt.text[:40])
    q2, _ = eg.planted(nt, rng, 200, [("i", 100)], p=12_000)
    q3 = bytes(nt.text[n - 30:n]) + b"AC"
    qs = [q0, q1, q2, q3, b"ACG", b"A" * 12]
    triples = []
    for qi in (0, 1, 2, 3):  # every true hit of the four reads
        p, d = er.hits_of(nt.t.D(qs[qi]), k)
        triples += [(qi, int(s), int(e)) for s, e in zip(p, d)]
    true = len(triples)
    assert true >= 4 and (0, 5000, 2) in triples and (1, 0, 0) in triples and (2, 12_000, 1) in triples
    # not a hit, but an alignment at that distance: the start before a hit, one edit dearer (its script begins with 'D')
    assert int(nt.t.D(q0)[4999]) == 3
    triples.append((0, 4999, 3))
    false = [(0, 5000, 1), (0, 5000, 3), (2, 12_000, 0),   # a wrong distance
             (0, 7000, 2), (1, 300, 0), (5, 100, 3),       # a start that is no hit
             (0, n, 2), (1, n + 7, 0),                     # a start >= n
             (4, 100, 0), (0, 5000, 4)]                    # a query not longer than k; a distance above max_edits
    triples += false
    tl, n_ops, ops, t = dev_align(nt, qs, triples, k, tally=True)
    aligned, cells = 0, 0
    for h, (qi, s, d) in enumerate(triples):
        wtl, wruns = al.align_triple(nt.t, qs[qi], s, d) if len(qs[qi]) > k and d <= k else (0, np.zeros(0, np.uint32))
        assert int(tl[h]) == wtl and int(n_ops[h]) == len(wruns), (h, qi, s, d)
        assert np.array_equal(ops[h, :len(wruns)], wruns), (h, cigar_string(ops[h, :n_ops[h]]), cigar_string(wruns))
        aligned += len(wruns) > 0
        L = len(qs[qi])
        if L > k and d <= k and s < n:
            J = min(L + d, n - s)
            cells += sum(max(0, min(J, i + d) - max(0, i - d) + 1) for i in range(L + 1))
    assert np.all(n_ops[:true] > 0) and n_ops[true] > 0 and cigar_string(ops[true, :n_ops[true]]).startswith("1D")
    assert not n_ops[true + 1:].any() and not tl[true + 1:].any()
    assert aligned == true + 1 and [int(v) for v in t] == [aligned, cells]
    again = dev_align(nt, qs, triples, k)
    assert np.array_equal(again[0], tl) and np.array_equal(again[1], n_ops)
    for h in range(len(triples)):
        assert np.array_equal(again[2][h, :n_ops[h]], ops[h, :n_ops[h]])


CPP = r'''
#include <cstdio>
#include <fstream>
#include <string>
#include <vector>
#include "awry.hpp"
int main(int argc, char** argv) {
  awry::FmBuildArgs a;
  a.input_file_src = argv[1];
  a.suffix_array_compression_ratio = 8;
  a.lookup_table_kmer_len = 5;
  try {
    awry::FmIndex ix = awry::FmIndex::create(a, {0});
    std::vector<std::string> qs;
    { std::ifstream f(argv[2]); std::string s; while (std::getline(f, s)) qs.push_back(s); }
    std::vector<uint8_t> status;
    auto al = ix.parallel_align_edit(qs, 3, 1000000, &status);
    auto loc = ix.parallel_locate_edit(qs, 3, 1000000);
    if (al.size() != qs.size() || status.size() != qs.size()) return 3;
    std::FILE* out = std::fopen(argv[3], "w");
    for (size_t i = 0; i < qs.size(); i++) {
      if (al[i].size() != loc[i].size() || status[i] != AWRY_Q_OK) return 4;
      for (size_t j = 0; j < al[i].size(); j++) {
        const awry::FmIndex::EditAlignment& h = al[i][j];
        if (h.global_position != loc[i][j].global_position || h.edits != loc[i][j].edits || !(h.position == loc[i][j].position)) return 5;
        if (h.cigar.empty() || h.cigar.size() > AWRY_ALIGN_MAX_OPS) return 6;
        std::fprintf(out, "%zu %llu %u %u %s\n", i, (unsigned long long)h.global_position, (unsigned)h.edits, (unsigned)h.text_len, h.cigar_string().c_str());
      }
    }
    std::fclose(out);
  } catch (const awry::Error& e) {
    std::printf("unexpected: %d %s\n", e.code, e.what());
    return 8;
  }
  std::puts("cpp-align-ok");
  return 0;
}
'''


def test_cpp_mirror_on_one_small_batch(nt, tmp_path):
    rng = np.random.default_rng(280)
    fa = str(tmp_path / "t.fa")
    synth.write_fasta(fa, nt.text, [int(s) for s in nt.st], ["seq%d" % i for i in range(len(nt.st))], 60)
    qs = eg.reads_for(nt, rng, 101, 3)[0][:8] + eg.reads_for(nt, rng, 33, 3)[0][:4]
    (tmp_path / "q.txt").write_bytes(b"\n".join(qs) + b"\n")
    src = tmp_path / "t.cpp"
    src.write_text(CPP)
    exe = tmp_path / "t"
    libdir = os.path.dirname(awry_amd.lib_path())
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L", libdir, "-lawry_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([str(exe), fa, str(tmp_path / "q.txt"), str(tmp_path / "out.txt")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "cpp-align-ok" in r.stdout, (r.returncode, r.stdout, r.stderr[-2000:])
    off, g, d, _, tl, coff, cg = al.align(nt.t, qs, 3, 10 ** 6)
    want = ["%d %d %d %d %s" % (i, int(g[h]), int(d[h]), int(tl[h]), cigar_string(cg[coff[h]:coff[h + 1]]))
            for i in range(len(qs)) for h in range(int(off[i]), int(off[i + 1]))]
    assert len(want) >= len(qs) and (tmp_path / "out.txt").read_text().splitlines() == want
    assert nt.ix.align_string_edit(qs[0], 3, NO_CAP) == nt.ix.parallel_align_edit(qs[:1], 3, NO_CAP)[0]
    per = nt.ix.parallel_align_edit(qs[:2], 3, NO_CAP)
    assert [(x[1], x[2], x[3]) for x in per[0]] == [(int(d[h]), int(tl[h]), cigar_string(cg[coff[h]:coff[h + 1]])) for h in range(int(off[0]), int(off[1]))]
