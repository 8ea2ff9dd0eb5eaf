"""CPU checks of tests/kmer_table_ref.py, the host recomputation the GPU audit of the k-mer count table rests on: its kt_mix is
the bijection of layout.h (against the C++ itself), its reference_table agrees with the oracle's counts, and the entry point
that lets a test read the table (awry_debug_kmer_table) is declared, exported and mirrored."""
import os
import re
import subprocess

import numpy as np

from awry_amd import _lib
from awry_amd.fm_index import FmIndex
from tests import kmer_table_ref as ref
from tests import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MIX_SRC = r'''
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "layout.h"
int main(int argc, char** argv) {
  if (argc != 4) return 2;
  const int L = std::atoi(argv[1]);
  FILE* in = std::fopen(argv[2], "rb");
  FILE* out = std::fopen(argv[3], "wb");
  if (!in || !out) return 3;
  std::vector<uint64_t> w(1 << 12);
  size_t n;
  while ((n = std::fread(w.data(), 8, w.size(), in)) > 0) {
    for (size_t j = 0; j < n; j++) w[j] = awry::kt_mix(w[j], L);
    if (std::fwrite(w.data(), 8, n, out) != n) return 4;
  }
  std::fclose(in);
  if (std::fclose(out) != 0) return 5;
  static_assert(awry::KT_CNT_BITS == 20 && awry::KT_TAG_SHIFT == 21 && awry::KT_ASK == (1ull << 20) - 1 && awry::KT_OVERFLOW == 1ull << 20, "layout");
  static_assert(awry::KT_TAG_NONE == (1ull << 43) - 1, "layout");
  return 0;
}
'''


def test_kt_mix_is_a_permutation_of_all_words():
    for L in (4, 7, 8):
        n = 1 << (2 * L)
        mx = ref.kt_mix(np.arange(n, dtype=np.uint64), L)
        assert np.array_equal(np.sort(mx), np.arange(n, dtype=np.uint64)), L


def test_kt_mix_stays_inside_its_word():
    rng = np.random.default_rng(1)
    for L in (21, 31, 32):
        w = rng.integers(0, 1 << 63, size=100_000, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=100_000, dtype=np.uint64)
        if L < 32:
            w &= np.uint64((1 << (2 * L)) - 1)
        mx = ref.kt_mix(w, L)
        if L < 32:
            assert (mx < np.uint64(1 << (2 * L))).all(), L
        assert len(np.unique(mx)) == len(np.unique(w)), L  # (no two of the sample collide)


def test_kt_mix_equals_the_cpp(tmp_path):
    src, exe = tmp_path / "mix.cpp", tmp_path / "mix"
    src.write_text(MIX_SRC)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "awry_amd", "csrc"), str(src), "-o", str(exe)])
    rng = np.random.default_rng(2)
    for L in (9, 21, 31, 32):
        w = rng.integers(0, 1 << 63, size=10_000, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=10_000, dtype=np.uint64)
        if L < 32:
            w &= np.uint64((1 << (2 * L)) - 1)
        w[:3] = [0, 1, (1 << (2 * L)) - 1]
        fin, fout = tmp_path / ("in%d" % L), tmp_path / ("out%d" % L)
        w.tofile(fin)
        subprocess.check_call([str(exe), str(L), str(fin), str(fout)], timeout=60)
        assert np.array_equal(np.fromfile(fout, dtype=np.uint64), ref.kt_mix(w, L)), L


def test_constants_are_the_header_s():
    src = open(os.path.join(ROOT, "awry_amd", "csrc", "layout.h")).read()
    assert "constexpr int KT_CNT_BITS = 20, KT_TAG_SHIFT = 21, KT_TAG_BITS = 64 - KT_TAG_SHIFT;" in src
    assert (ref.KT_CNT_BITS, ref.KT_TAG_SHIFT, ref.KT_TAG_BITS, ref.KT_ASK, ref.KT_OVERFLOW, ref.KT_TAG_NONE) == (20, 21, 43, (1 << 20) - 1, 1 << 20, (1 << 43) - 1)
    lcx = open(os.path.join(ROOT, "awry_amd", "csrc", "kernels_nt2_kmer.hip.h")).read()
    assert re.search(r"LCX_LANE_ROWS\s*=\s*4\b", lcx), "the reference covers the buckets of more than LCX_LANE_ROWS rows"


def test_reference_table_agrees_with_the_oracle(oracle):
    from tests.test_lcx_gpu import family_text
    text, st, hd = family_text(200_000, 6, [(300, 160, 0.10), (120, 400, 0.03), (40, 130, 0.0)], 3, 0.02)
    oi = oracle.OracleIndex.from_text(text, 0, 8, 0, st, hd)
    try:
        rng = np.random.default_rng(3)
        for k, L in ((9, 21), (9, 10), (8, 31), (10, 32)):
            words, counts = ref.reference_table(text, k, L)
            assert len(words) > 3000 and np.array_equal(words, np.unique(words)), (k, L, len(words))
            table = dict(zip(words.tolist(), counts.tolist()))
            pres = synth.sampled_queries(text, 2000, L, 10 + L)
            want, _ = oi.parallel_count(*synth.fixed_to_csr(pres), 4)
            rows, _ = oi.parallel_count(*synth.fixed_to_csr(np.ascontiguousarray(pres[:, L - k:])), 4)
            got = np.array([table.get(w, 0) for w in ref.pack_queries(pres).tolist()], dtype=np.uint64)
            covered = rows > ref.LANE_ROWS
            assert covered.sum() > 300 and (~covered).sum() > 300, (k, L, int(covered.sum()))
            assert np.array_equal(got[covered], want[covered]), (k, L)
            assert (got[~covered] == 0).all(), ("an L-mer of a bucket of at most 4 rows is not in the table", k, L)
            # and from the other side: keys drawn from the reference count as it says
            pick = rng.integers(0, len(words), size=2000)
            q = synth.NT[((words[pick][:, None] >> (2 * np.arange(L, dtype=np.uint64))[None, :]) & np.uint64(3)).astype(np.int64)]
            want, _ = oi.parallel_count(*synth.fixed_to_csr(q), 4)
            assert np.array_equal(want.astype(np.int64), counts[pick]), (k, L)
    finally:
        oi.close()


def test_expected_lines_and_audit_on_a_handmade_table():
    """audit() passes on a table filled by the definition and fails on each single defect it is there to find"""
    import pytest
    rng = np.random.default_rng(4)
    L, bits = 12, 6
    words = np.unique(rng.integers(0, 1 << (2 * L), size=900, dtype=np.uint64))
    counts = rng.integers(1, 50, size=len(words)).astype(np.int64)
    counts[:3] = [ref.KT_ASK - 1, ref.KT_ASK, ref.KT_ASK + 5]
    line, tag, storable, n_store, marked = ref.expected_lines(words, L, bits)
    assert storable.all() and 0.2 < marked.mean() < 0.8 and n_store.sum() == len(words)
    tab = np.zeros((1 << bits, 16), dtype=np.uint64)
    fill = np.zeros(1 << bits, dtype=np.int64)
    for j in rng.permutation(len(words)).tolist():
        ln = int(line[j])
        if fill[ln] < 16:
            tab[ln, fill[ln]] = (int(tag[j]) << ref.KT_TAG_SHIFT) | min(int(counts[j]), ref.KT_ASK)
            fill[ln] += 1
    tab[marked, 0] |= np.uint64(ref.KT_OVERFLOW)
    entries, n_marked = ref.audit(tab.reshape(-1), bits, L, words, counts)
    assert entries == int(np.minimum(n_store, 16).sum()) and n_marked == int(marked.sum())
    un = int(np.flatnonzero(~marked & (n_store >= 2))[0])
    mk = int(np.flatnonzero(marked)[0])

    def broken(edit):
        t = tab.copy()
        edit(t)
        with pytest.raises(AssertionError):
            ref.audit(t.reshape(-1), bits, L, words, counts)

    broken(lambda t: t.__setitem__((un, 0), 0))                                        # an entry lost
    broken(lambda t: t.__setitem__((un, 1), t[un, 1] + np.uint64(1)))                  # a count off by one
    broken(lambda t: t.__setitem__((mk, 0), t[mk, 0] & ~np.uint64(ref.KT_OVERFLOW)))   # a mark missing
    broken(lambda t: t.__setitem__((un, 0), t[un, 0] | np.uint64(ref.KT_OVERFLOW)))    # a mark too many
    broken(lambda t: t.__setitem__((un, 1), t[un, 1] | np.uint64(ref.KT_OVERFLOW)))    # bit 20 outside slot 0
    broken(lambda t: t.__setitem__((un, 15), t[un, 0] & ~np.uint64(ref.KT_OVERFLOW)))  # a tag twice in a line
    broken(lambda t: t.__setitem__((un, 15), (np.uint64(12345) << np.uint64(ref.KT_TAG_SHIFT)) | np.uint64(1)))  # a stranger
    broken(lambda t: t.__setitem__((mk, 15), 0))                                       # a marked line not full


def test_the_debug_entry_point_is_declared_exported_and_mirrored():
    L = _lib.load_library()
    name = "awry_debug_kmer_table"
    assert name in _lib.header_symbols()
    assert getattr(L, name) is not None
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "awry_hip.h")).read(), flags=re.S)
    args = re.search(r"\b%s\s*\(([^)]*)\)" % name, src).group(1)
    assert " ".join(args.split()) == "awry_index_t *idx, int slot, uint64_t *host_out, uint64_t capacity_words, int *L_out, uint32_t *bits_out"
    assert len(args.split(",")) == len(getattr(L, name).argtypes) == 6
    rust = open(os.path.join(ROOT, "rust", "awry-hip-sys", "src", "lib.rs")).read()
    assert "pub fn awry_debug_kmer_table(idx: *mut awry_index_t, slot: c_int, host_out: *mut u64, capacity_words: u64, L_out: *mut c_int, bits_out: *mut u32) -> c_int;" in rust
    assert "`awry_debug_kmer_table(" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert callable(FmIndex.debug_kmer_table)
    # without a replica there is nothing to read, and the call says so
    import ctypes as C

    from awry_amd.fm_index import ERR_NO_DEVICE, AwryError
    text, st, hd = synth.make_text(300, 0, 1)
    ix = FmIndex.from_text(text, 0, 8, 0, st, hd)
    try:
        ix.debug_kmer_table()
        raise AssertionError("no replica: the call must fail")
    except AwryError as e:
        assert e.code == ERR_NO_DEVICE
    assert L.awry_debug_kmer_table(None, 0, None, 0, C.byref(C.c_int()), C.byref(C.c_uint32())) != 0
