// awry_hip.hip -- C ABI (include/awry_hip.h) over the gfx950 kernels: device replicas, batch drivers,
// seed-table construction.  There is deliberately no CPU implementation of count / locate here.
#include "dev_common.h"
#include "replica.h"
#include "accelerators.h"
#include "launchers.h"
#include "host_count.h"
#include "host_locate.h"
#include "batch_host.h"
#include "mismatch_host.h"
#include "anchor_host.h"
#include "chain_host.h"
#include "edit_host.h"
#include "chain_align_host.h"
#include "map_host.h"
#include "split_host.h"
#include "pair_host.h"
#include "prewarm.h"

namespace {

// small result arrays of the single-query entry points (awry_locate): plain heap memory, which awry_free_buffer tells
// apart from the pinned pool blocks of the batch paths (release_result); large ones 2 MB-aligned and advised for huge pages
template <class T>
T* malloc_array(size_t n) {
  const size_t bytes = std::max<size_t>(1, n) * sizeof(T);
  void* p = nullptr;
  if (bytes >= (8u << 20)) {
    if (posix_memalign(&p, 2u << 20, bytes) != 0) p = nullptr;
    if (p) (void)madvise(p, bytes, MADV_HUGEPAGE);
  } else p = malloc(bytes);
  if (!p) throw std::bad_alloc();
  return static_cast<T*>(p);
}

void fill_ref_kmer_table(awry_index* ix) {
  HostIndex& h = ix->host;
  const uint64_t nslots = ref_kmer_table_entries(h.alphabet, h.kmer_len);
  if (h.ref_kmer_table.size() == 2 * nslots) return;
  if (ix->reps.empty()) {  // saving is host work: no replica, no GPU needed
    fill_ref_kmer_table_host(h);
    return;
  }
  Replica& r = replica(ix, 0);
  DevBuf<uint64_t> tab(2 * nslots);
  const dim3 g(grid_for(r, nslots, 256)), b(256);
  with_alphabet(h.alphabet, [&](auto A) { hipLaunchKernelGGL(ref_kmer_table_kernel<A()>, g, b, 0, r.stream, r.dev, (int)h.kmer_len, nslots, tab.p); });
  HIP_CHECK(hipGetLastError());
  h.ref_kmer_table.resize(2 * nslots);
  HIP_CHECK(hipMemcpyAsync(h.ref_kmer_table.data(), tab.p, 2 * nslots * 8, hipMemcpyDeviceToHost, r.stream));
  HIP_CHECK(hipStreamSynchronize(r.stream));
}

uint64_t scalar_op(awry_index* ix, int op, uint64_t a, uint64_t b, int idx, uint64_t* second = nullptr) {
  Replica& r = replica(ix, 0);
  DevBuf<uint64_t> out(2);
  with_alphabet(r.dev.alphabet, [&](auto A) { hipLaunchKernelGGL(scalar_ops_kernel<A()>, dim3(1), dim3(64), 0, r.stream, r.dev, op, a, b, idx, out.p); });
  HIP_CHECK(hipGetLastError());
  uint64_t h[2] = {0, 0};
  HIP_CHECK(hipMemcpyAsync(h, out.p, 16, hipMemcpyDeviceToHost, r.stream));
  HIP_CHECK(hipStreamSynchronize(r.stream));
  if (second) *second = h[1];
  return h[0];
}

int checked_symbol(const awry_index* ix, uint8_t ascii) {
  if (ascii >= 0x80) throw QueryError("non-ASCII symbol");
  return index_of_ascii(ix->host.alphabet, ascii);
}

// awry_dev_pair_windows and its clipped mode: Rec is the kernels' record of the caller's MapT
template <class Rec, class MapT>
void dev_pair_windows(awry_index_t* idx, int slot, const uint64_t* d_cand_off, const MapT* d_cands, const uint64_t* d_qoff, uint64_t n_pairs,
                      uint64_t min_insert, uint64_t max_insert, uint32_t rescue_anchors, int rescue_edits, uint32_t* d_win_query, uint64_t* d_win_first,
                      uint32_t* d_win_count, void* stream) {
  const PairParams pp = pair_params(min_insert, max_insert, 0, rescue_anchors, rescue_edits);
  require(idx != nullptr, "null argument");
  if (idx->host.alphabet != NUCLEOTIDE) throw ArgError("mapping read pairs needs a nucleotide index");
  Replica& r = replica(idx, slot);
  require_chain_index(r.dev.bwt_len);
  require(n_pairs < (1ull << 28), "more than 2^28 - 1 pairs in one launch");
  require(n_pairs == 0 || rescue_anchors == 0 || (d_cand_off && d_cands && d_qoff && d_win_query && d_win_first && d_win_count), "null device pointer");
  launch_pair_windows(r, d_cand_off, reinterpret_cast<const Rec*>(d_cands), d_qoff, 1, n_pairs, pp, d_win_query, d_win_first, d_win_count,
                      (hipStream_t)stream);
}

// awry_dev_pair_select and its clipped mode
template <class Rec, class MapT>
void dev_pair_select(awry_index_t* idx, int slot, const uint64_t* d_cand_off, const MapT* d_cands, const MapT* d_resc, const uint8_t* d_read_status,
                     uint64_t n_pairs, const PairParams& pp, const PairMode& pm, uint64_t* d_n_maps, const uint64_t* d_map_off, MapT* d_maps, uint32_t* d_sel,
                     awry_pos_t* d_pos, uint32_t* d_insert, void* stream) {
  require(idx != nullptr, "null argument");
  if (idx->host.alphabet != NUCLEOTIDE) throw ArgError("mapping read pairs needs a nucleotide index");
  Replica& r = replica(idx, slot);
  require(n_pairs < (1ull << 28), "more than 2^28 - 1 pairs in one launch");
  require(n_pairs == 0 || (d_cand_off && d_cands && (pp.rescue_anchors == 0 || d_resc) && (d_map_off ? d_maps != nullptr : d_n_maps != nullptr)),
          "null device pointer");
  launch_pair_select<Rec>(r, d_cand_off, reinterpret_cast<const Rec*>(d_cands), pp.rescue_anchors ? reinterpret_cast<const Rec*>(d_resc) : nullptr,
                          d_read_status, n_pairs, pp, pm, d_n_maps, d_map_off, reinterpret_cast<Rec*>(d_maps), d_sel, reinterpret_cast<uint64_t*>(d_pos),
                          d_insert, (hipStream_t)stream);
}

}  // namespace

// =====================================================================================================
// C ABI
// =====================================================================================================
extern "C" {

const char* awry_last_error(void) { return g_last_error.c_str(); }

// build_device: >= 0 construct on that GPU (sa_builder.hip); AWRY_BUILD_HOST (-1) host SA-IS;
// AWRY_BUILD_AUTO (-2): GPU 0 when one is visible and the text is large enough to pay for it
// The index is built over the CANONICAL text: every byte replaced by the letter of its symbol index (lower case folded,
// U -> T, IUPAC codes and anything else -> N; non-standard residues -> X) -- the map queries go through
// (src/alphabet.rs:109-114,169-248).  Suffixes must be sorted in the order the BWT encodes them: sorted by raw bytes, a
// text with R / Y / K ... (or B / Z / U / O / J in proteins) would put its N- (X-) suffixes in several places while
// prefix_sums assume one block, and LF steps and text comparison would disagree.  Returns true and fills `out` when the
// text had to be rewritten.  An inner '$' / '#' is an argument error (the text model has exactly one sentinel, at the end).
static bool canonical_text(const uint8_t* text, uint64_t bwt_len, int alphabet, std::vector<uint8_t>& out) {
  uint8_t canon[256];
  for (int b = 0; b < 256; b++) canon[b] = ascii_of_index(alphabet, index_of_ascii(alphabet, (uint8_t)b));
  const uint64_t body = bwt_len - 1;
  std::atomic<int> other{0}, sentinel{0};
  HostPool::instance().run_ranges(body, 1u << 22, [&](uint64_t lo, uint64_t hi) {
    unsigned diff = 0, sent = 0;
    for (uint64_t i = lo; i < hi; i++) {  // branch-free: vectorises
      const uint8_t c = canon[text[i]];
      diff |= (unsigned)(c != text[i]);
      sent |= (unsigned)(c == '$');
    }
    if (diff) other.store(1, std::memory_order_relaxed);
    if (sent) sentinel.store(1, std::memory_order_relaxed);
  });
  if (sentinel.load()) throw ArgError("the text holds '$' or '#' before its last byte (the text model has one sentinel, at the end)");
  if (!other.load()) return false;
  out.resize(bwt_len);
  HostPool::instance().run_ranges(body, 1u << 22, [&](uint64_t lo, uint64_t hi) {
    for (uint64_t i = lo; i < hi; i++) out[i] = canon[text[i]];
  });
  out[body] = '$';
  return true;
}

static void construct(awry_index* ix, const uint8_t* text, uint64_t bwt_len, int alphabet, uint64_t sa_ratio, uint8_t kmer_len,
                      const uint64_t* seq_starts, const char* const* headers, uint64_t nseq, int build_device) {
  static const uint64_t zero = 0;
  if (nseq == 0 || !seq_starts) { seq_starts = &zero; nseq = 1; headers = nullptr; }
  if (bwt_len == 0 || text[bwt_len - 1] != '$') throw ArgError("text must end with '$'");
  std::vector<uint8_t> canon;
  if (canonical_text(text, bwt_len, alphabet, canon)) text = canon.data();
  const bool automatic = build_device == AWRY_BUILD_AUTO;
  if (build_device == AWRY_BUILD_AUTO) {
    const char* e = getenv("AWRY_BUILD");
    int ndev = 0;
    if (e && !strcmp(e, "host")) build_device = AWRY_BUILD_HOST;
    else if (hipGetDeviceCount(&ndev) == hipSuccess && ndev > 0 && bwt_len < (1ull << 32) - 1 && (bwt_len >= (1u << 20) || (e && !strcmp(e, "gpu")))) {
      // the calling thread's current device (one process per GPU sets it to its own), else GPU 0
      if (hipGetDevice(&build_device) != hipSuccess || build_device < 0 || build_device >= ndev) build_device = 0;
    } else build_device = AWRY_BUILD_HOST;
  }
  if (build_device < 0) {
    build_from_text(ix->host, text, bwt_len, alphabet, sa_ratio, kmer_len, seq_starts, headers, nseq);
    return;
  }
  prepare_build(ix->host, text, bwt_len, alphabet, sa_ratio, kmer_len, seq_starts, headers, nseq);
  try {
    gpu_build_index(ix->host, text, bwt_len, build_device, getenv("AWRY_VERBOSE") != nullptr);
  } catch (const std::bad_alloc&) {
    throw;
  } catch (const std::exception& e) {
    // Construction is host work in the reference; the GPU is how it gets fast here, not a requirement.  When the device
    // was chosen automatically and cannot do it (its HBM is taken by replicas, say: the builder needs ~45 B per symbol),
    // the host builder produces the same index, only slower.  An explicit device request fails loudly instead.
    if (!automatic) throw HipError(std::string("GPU index construction: ") + e.what());
    (void)hipGetLastError();
    if (getenv("AWRY_VERBOSE")) fprintf(stderr, "[awry] GPU index construction failed (%s): building on the host\n", e.what());
    ix->host = HostIndex();
    build_from_text(ix->host, text, bwt_len, alphabet, sa_ratio, kmer_len, seq_starts, headers, nseq);
  }
}

int awry_build_from_text_on(const uint8_t* text, uint64_t bwt_len, int alphabet, uint64_t sa_ratio, uint8_t kmer_len,
                            const uint64_t* seq_starts, const char* const* headers, uint64_t nseq, int build_device,
                            awry_index_t** out) {
  return guarded([&] {
    require(text && out && bwt_len > 0, "null argument");
    require(alphabet == NUCLEOTIDE || alphabet == AMINO, "bad alphabet id");
    require(build_device >= AWRY_BUILD_AUTO, "bad build device");
    auto ix = std::make_unique<awry_index>();
    construct(ix.get(), text, bwt_len, alphabet, sa_ratio, kmer_len, seq_starts, headers, nseq, build_device);
    *out = ix.release();
  });
}

int awry_build_from_text(const uint8_t* text, uint64_t bwt_len, int alphabet, uint64_t sa_ratio, uint8_t kmer_len,
                         const uint64_t* seq_starts, const char* const* headers, uint64_t nseq, awry_index_t** out) {
  return awry_build_from_text_on(text, bwt_len, alphabet, sa_ratio, kmer_len, seq_starts, headers, nseq, AWRY_BUILD_AUTO, out);
}

int awry_build(const awry_build_args_t* args, awry_index_t** out) {
  return guarded([&] {
    require(args && args->input_path && out, "null argument");
    require(args->alphabet <= 1, "bad alphabet id");
    SequenceFile sf = read_sequence_file(args->input_path, args->alphabet);
    std::vector<const char*> hdr;
    for (auto& h : sf.headers) hdr.push_back(h.c_str());
    auto ix = std::make_unique<awry_index>();
    construct(ix.get(), sf.text.data(), sf.text.size(), args->alphabet, args->sa_ratio, args->kmer_len, sf.starts.data(),
              hdr.data(), sf.starts.size(), AWRY_BUILD_AUTO);
    *out = ix.release();
  });
}

int awry_load(const char* path, awry_index_t** out) {
  return guarded([&] {
    require(path && out, "null argument");
    auto ix = std::make_unique<awry_index>();
    load_awry(ix->host, path);
    *out = ix.release();
  });
}

int awry_save(awry_index_t* idx, const char* path) {
  return guarded([&] {
    require(idx && path, "null argument");
    fill_ref_kmer_table(idx);
    save_awry(idx->host, path);
  });
}

void awry_free(awry_index_t* idx) { delete idx; }

int awry_set_devices(awry_index_t* idx, const int* device_ids, int n_devices) {
  return guarded([&] {
    require(idx != nullptr, "null index");
    if (n_devices <= 0 || !device_ids) throw NoDeviceError("awry_set_devices needs at least one GPU: there is no CPU search path");
    // the old replicas go first: the policies below size the seed table and the accelerators from the HBM that is free,
    // and a rebuilt replica on the same GPU must not see half of it (if the build fails the index is left without replicas)
    idx->reps.clear();
    std::vector<std::unique_ptr<Replica>> reps(n_devices);
    if (n_devices == 1) {
      reps[0] = make_replica(idx, device_ids[0]);
    } else {  // one host thread per GPU: upload + seed-table build run concurrently on all of them
      std::vector<std::exception_ptr> errs(n_devices);
      std::vector<std::thread> pool;
      for (int i = 0; i < n_devices; i++)
        pool.emplace_back([&, i] {
          try { reps[i] = make_replica(idx, device_ids[i]); } catch (...) { errs[i] = std::current_exception(); }
        });
      for (auto& t : pool) t.join();
      for (auto& e : errs) if (e) std::rethrow_exception(e);
    }
    idx->reps = std::move(reps);
    for (auto& r : idx->reps) prewarm_host_paths(*r);
  });
}

int awry_set_seed_kmer_len(awry_index_t* idx, int k) {
  return guarded([&] {
    require(idx != nullptr, "null index");
    require(k >= -1 && k <= 17, "seed k-mer length must be in -1..17 (amino: ..7)");
    idx->seed_k_request = k;
    change_replicas(idx, [&](Replica& r) { rebuild_seed(idx, r, wanted_seed_k(idx)); });
  });
}

int awry_debug_set_count_kernel(int mode) { g_count_kernel.store(mode); return AWRY_OK; }
int awry_debug_force_wide_rows(int on) { g_force_wide.store(on ? 1 : 0); return AWRY_OK; }
int awry_debug_set_max_blocks(int blocks) {
  if (blocks < 0) { g_last_error = "awry_debug_set_max_blocks: negative bound"; return AWRY_ERR_ARG; }
  g_max_blocks.store(blocks);
  return AWRY_OK;
}
int awry_debug_max_blocks(void) { return g_max_blocks.load(); }

const char* awry_count_schedule(const awry_index_t* idx, int L) {
  if (!idx || idx->reps.empty()) return "";
  // the plan of a seeded launch without census whose batch is at or above every batch-size threshold (rung, count table)
  const CountFacts f = count_facts(*idx->reps[0]);
  const uint64_t n = 1u << 20;
  return plan_name(L > 32 ? plan_reads(f, n, L, true, false) : plan_kmers(f, n, L, true, false));
}

int awry_seed_kmer_len(const awry_index_t* idx) { return idx && !idx->reps.empty() ? idx->reps[0]->seed_k : 0; }
int awry_num_devices(const awry_index_t* idx) { return idx ? (int)idx->reps.size() : 0; }
int awry_replica_device(const awry_index_t* idx, int slot) {
  return idx && slot >= 0 && slot < (int)idx->reps.size() ? idx->reps[slot]->device : -1;
}

int awry_count_batch(awry_index_t* idx, const uint8_t* qbytes, const uint64_t* qoff, uint64_t n, uint64_t* counts_out) {
  return guarded([&] {
    require(idx && qoff && (counts_out || n == 0), "null argument");
    require(qbytes || qoff[n] == qoff[0], "null query bytes");
    const auto t0 = std::chrono::steady_clock::now();
    for_each_replica(idx, n, [&](Replica& r, Shard sh, int) { count_shard(r, qbytes, qoff, sh, counts_out); });
    if (getenv("AWRY_TRACE_HOST"))
      fprintf(stderr, "[awry] awry_count_batch %.2f ms\n", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
  });
}

// k-mers that the caller already holds packed (letter j of a k-mer in bits [2j, 2j + 2) of its word, A0 C1 G2 T3): no
// ASCII crosses PCIe, 16 B per query both ways instead of L + 8.
int awry_count_packed_kmers(awry_index_t* idx, const uint64_t* words, uint64_t n, int L, uint64_t* counts_out) {
  return guarded([&] {
    require(idx && ((words && counts_out) || n == 0), "null argument");
    require(L >= 1 && L <= 32, "packed k-mer length must be in 1..32");
    for_each_replica(idx, n, [&](Replica& r, Shard sh, int) {
      HIP_CHECK(hipSetDevice(r.device));
      require(r.dev.alphabet == NUCLEOTIDE, "packed k-mers need a nucleotide index");
      if (sh.hi <= sh.lo) return;
      PackedPlan plan;
      plan.ok = true;
      plan.Lmax = (uint64_t)L;
      count_shard_hostpacked(r, nullptr, nullptr, sh, plan, counts_out, words);  // staged through the lanes' pinned buffers
    });
  });
}

int awry_locate_batch(awry_index_t* idx, const uint8_t* qbytes, const uint64_t* qoff, uint64_t n, uint64_t** hit_off_out,
                      awry_pos_t** hits_out, uint64_t** global_pos_out) {
  return guarded([&] {
    require(idx && qoff && hit_off_out, "null argument");
    require(qbytes || qoff[n] == qoff[0], "null query bytes");
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<LocateResult> res(std::max<size_t>(1, idx->reps.size()));
    for (auto& x : res) x.want_pos = hits_out != nullptr;
    MBuf<uint64_t> off;  // pinned (PinnedPool): the shards' device scans are copied straight into it
    off.grow(n + 1);
    off.p[0] = 0;
    {
      auto shards = shard_queries(n, res.size());  // the same cut for_each_replica makes
      for (size_t g = 0; g < res.size(); g++) res[g].off = off.p + shards[g].lo;
    }
    for_each_replica(idx, n, [&](Replica& r, Shard sh, int g) { locate_shard(r, qbytes, qoff, sh, global_pos_out != nullptr, res[g]); });
    uint64_t total = 0;
    for (size_t g = 0; g < res.size(); g++) {  // shards are contiguous in query order: rebase every shard after the first
      if (g && total)
        for (uint64_t i = 1; i <= res[g].nq; i++) res[g].off[i] += total;
      total += res[g].total;
    }
    if (res.size() == 1 && (!hits_out || res[0].pos.p) && (!global_pos_out || res[0].gpos.p)) {  // one replica: its arrays are the result
      if (hits_out) *hits_out = res[0].pos.release();
      if (global_pos_out) *global_pos_out = res[0].gpos.release();
    } else {
      MBuf<awry_pos_t> hits;
      MBuf<uint64_t> gp;
      if (hits_out) hits.grow(std::max<uint64_t>(1, total));
      if (global_pos_out) gp.grow(std::max<uint64_t>(1, total));
      uint64_t at = 0;
      for (auto& x : res) {
        if (hits_out && x.total) pool_memcpy(hits.p + at, x.pos.p, x.total * sizeof(awry_pos_t));
        if (global_pos_out && x.total) pool_memcpy(gp.p + at, x.gpos.p, x.total * 8);
        at += x.total;
      }
      if (hits_out) *hits_out = hits.release();
      if (global_pos_out) *global_pos_out = gp.release();
    }
    *hit_off_out = off.release();
    if (getenv("AWRY_TRACE_HOST"))
      fprintf(stderr, "[awry] awry_locate_batch %.2f ms\n", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
  });
}

void awry_free_buffer(void* p) { release_result(p); }

int awry_count_mismatch_batch(awry_index_t* idx, const uint8_t* qbytes, const uint64_t* qoff, uint64_t n, int max_mismatches,
                              uint64_t* counts_out) {
  return guarded([&] { count_leaves_batch(idx, qbytes, qoff, n, max_mismatches, counts_out, false); });
}

int awry_locate_mismatch_batch(awry_index_t* idx, const uint8_t* qbytes, const uint64_t* qoff, uint64_t n, int max_mismatches,
                               uint64_t** hit_off_out, awry_pos_t** hits_out, uint64_t** global_pos_out, uint8_t** mismatches_out) {
  return guarded([&] {
    locate_leaves_batch(idx, qbytes, qoff, n, max_mismatches, hit_off_out, hits_out, global_pos_out, mismatches_out, false);
  });
}

uint32_t awry_pattern_class(int alphabet, uint8_t ascii) {
  return alphabet == AWRY_NUCLEOTIDE || alphabet == AWRY_AMINO ? pattern_class(alphabet, ascii) : 0;
}

int awry_count_pattern_batch(awry_index_t* idx, const uint8_t* qbytes, const uint64_t* qoff, uint64_t n, int max_mismatches,
                             uint64_t* counts_out) {
  return guarded([&] { count_leaves_batch(idx, qbytes, qoff, n, max_mismatches, counts_out, true); });
}

int awry_locate_pattern_batch(awry_index_t* idx, const uint8_t* qbytes, const uint64_t* qoff, uint64_t n, int max_mismatches,
                              uint64_t** hit_off_out, awry_pos_t** hits_out, uint64_t** global_pos_out, uint8_t** mismatches_out) {
  return guarded([&] {
    locate_leaves_batch(idx, qbytes, qoff, n, max_mismatches, hit_off_out, hits_out, global_pos_out, mismatches_out, true);
  });
}

int awry_anchor_batch(awry_index_t* idx, const uint8_t* qbytes, const uint64_t* qoff, uint64_t n, uint32_t min_len, int skip,
                      uint64_t** anchor_off_out, awry_anchor_t** anchors_out) {
  return guarded([&] {
    require(idx && qoff && anchor_off_out && anchors_out, "null argument");
    require(qbytes || qoff[n] == qoff[0], "null query bytes");
    require_anchor_args(min_len, skip);
    anchor_batch(idx, qbytes, qoff, n, anchor_finder(min_len, skip), 0, anchor_off_out, anchors_out, nullptr, nullptr, nullptr);
  });
}

int awry_locate_anchors_batch(awry_index_t* idx, const uint8_t* qbytes, const uint64_t* qoff, uint64_t n, uint32_t min_len, int skip,
                              uint64_t max_hits, uint64_t** anchor_off_out, awry_anchor_t** anchors_out, uint64_t** hit_off_out,
                              awry_pos_t** hits_out, uint64_t** global_pos_out) {
  return guarded([&] {
    require(idx && qoff && anchor_off_out && anchors_out && hit_off_out, "null argument");
    require(qbytes || qoff[n] == qoff[0], "null query bytes");
    require_anchor_args(min_len, skip);
    require(max_hits != 0, "max_hits must be at least 1 (a one-letter anchor has a quarter of the text as hits)");
    anchor_batch(idx, qbytes, qoff, n, anchor_finder(min_len, skip), max_hits, anchor_off_out, anchors_out, hit_off_out, hits_out, global_pos_out);
  });
}

int awry_smem_batch(awry_index_t* idx, const uint8_t* qbytes, const uint64_t* qoff, uint64_t n, uint32_t min_len, uint64_t** smem_off_out,
                    awry_anchor_t** smems_out) {
  return guarded([&] {
    require(idx && qoff && smem_off_out && smems_out, "null argument");
    require(qbytes || qoff[n] == qoff[0], "null query bytes");
    require_smem_args(min_len);
    anchor_batch(idx, qbytes, qoff, n, smem_finder(min_len), 0, smem_off_out, smems_out, nullptr, nullptr, nullptr);
  });
}

int awry_locate_smems_batch(awry_index_t* idx, const uint8_t* qbytes, const uint64_t* qoff, uint64_t n, uint32_t min_len, uint64_t max_hits,
                            uint64_t** smem_off_out, awry_anchor_t** smems_out, uint64_t** hit_off_out, awry_pos_t** hits_out,
                            uint64_t** global_pos_out) {
  return guarded([&] {
    require(idx && qoff && smem_off_out && smems_out && hit_off_out, "null argument");
    require(qbytes || qoff[n] == qoff[0], "null query bytes");
    require_smem_args(min_len);
    require(max_hits != 0, "max_hits must be at least 1 (a one-letter match has a quarter of the text as hits)");
    anchor_batch(idx, qbytes, qoff, n, smem_finder(min_len), max_hits, smem_off_out, smems_out, hit_off_out, hits_out, global_pos_out);
  });
}

int awry_chain_batch(awry_index_t* idx, const uint8_t* qbytes, const uint64_t* qoff, uint64_t n, uint32_t min_len, uint64_t max_hits, uint32_t max_seeds,
                     uint32_t lookback, uint32_t max_gap, uint32_t max_skew, uint32_t min_score, uint64_t** chain_off_out, awry_chain_t** chains_out,
                     uint64_t** seed_off_out, awry_seed_t** seeds_out, uint8_t** status_out) {
  return guarded([&] {
    const Reads q = checked_reads(idx, qbytes, qoff, n, chain_off_out);
    const Seeding sc(min_len, max_hits, max_seeds, lookback, max_gap, max_skew, min_score);
    require((seed_off_out == nullptr) == (seeds_out == nullptr), "seed_off_out and seeds_out are given or omitted together");
    chain_batch(idx, q, sc, chain_off_out, chains_out, seed_off_out, seeds_out, status_out);
  });
}

int awry_align_chains_batch(awry_index_t* idx, const uint8_t* qbytes, const uint64_t* qoff, uint64_t n, uint32_t min_len, uint64_t max_hits,
                            uint32_t max_seeds, uint32_t lookback, uint32_t max_gap, uint32_t max_skew, uint32_t min_score, uint64_t max_alignments,
                            uint32_t band, uint64_t** aln_off_out, awry_chain_t** chains_out, awry_aln_t** alns_out, uint64_t** cigar_off_out,
                            uint32_t** cigar_out, uint8_t** status_out) {
  return guarded([&] {
    const Reads q = checked_reads(idx, qbytes, qoff, n, aln_off_out);
    const Seeding sc(min_len, max_hits, max_seeds, lookback, max_gap, max_skew, min_score);
    require_chain_align_args(max_alignments, band);
    require_cigar_pair(cigar_off_out, cigar_out);
    align_chains_batch(idx, q, sc, max_alignments, band, AlignMode{}, AlnOut<awry_aln_t>{aln_off_out, chains_out, alns_out, cigar_off_out, cigar_out, status_out});
  });
}

int awry_align_chains_clip_batch(awry_index_t* idx, const uint8_t* qbytes, const uint64_t* qoff, uint64_t n, uint32_t min_len, uint64_t max_hits,
                                 uint32_t max_seeds, uint32_t lookback, uint32_t max_gap, uint32_t max_skew, uint32_t min_score, uint64_t max_alignments,
                                 uint32_t band, uint32_t match, uint32_t mismatch, uint32_t gap, uint32_t end_bonus, uint64_t** aln_off_out,
                                 awry_chain_t** chains_out, awry_aln_clip_t** alns_out, uint64_t** cigar_off_out, uint32_t** cigar_out, uint8_t** status_out) {
  return guarded([&] {
    const Reads q = checked_reads(idx, qbytes, qoff, n, aln_off_out);
    const Seeding sc(min_len, max_hits, max_seeds, lookback, max_gap, max_skew, min_score);
    require_chain_align_args(max_alignments, band);
    const AlignMode md = clip_mode(match, mismatch, gap, end_bonus);
    require_cigar_pair(cigar_off_out, cigar_out);
    align_chains_batch(idx, q, sc, max_alignments, band, md, AlnOut<awry_aln_clip_t>{aln_off_out, chains_out, alns_out, cigar_off_out, cigar_out, status_out});
  });
}

int awry_map_batch(awry_index_t* idx, const uint8_t* qbytes, const uint64_t* qoff, uint64_t n, uint32_t min_len, uint64_t max_hits, uint32_t max_seeds,
                   uint32_t lookback, uint32_t max_gap, uint32_t max_skew, uint32_t min_score, uint64_t chains_per_strand, uint64_t max_report, uint32_t band,
                   uint64_t** map_off_out, awry_map_t** maps_out, awry_pos_t** pos_out, uint64_t** cigar_off_out, uint32_t** cigar_out, uint8_t** status_out) {
  return guarded([&] {
    const Reads q = checked_reads(idx, qbytes, qoff, n, map_off_out);
    const Seeding sc(min_len, max_hits, max_seeds, lookback, max_gap, max_skew, min_score);
    require_map_args(chains_per_strand, max_report, band);
    require_cigar_pair(cigar_off_out, cigar_out);
    map_batch(idx, q, sc, (uint32_t)chains_per_strand, (uint32_t)max_report, band, AlignMode{}, MapMode{},
              MapOut<awry_map_t>{map_off_out, maps_out, pos_out, cigar_off_out, cigar_out, status_out});
  });
}

int awry_map_clip_batch(awry_index_t* idx, const uint8_t* qbytes, const uint64_t* qoff, uint64_t n, uint32_t min_len, uint64_t max_hits, uint32_t max_seeds,
                        uint32_t lookback, uint32_t max_gap, uint32_t max_skew, uint32_t min_score, uint64_t chains_per_strand, uint64_t max_report,
                        uint32_t band, uint32_t match, uint32_t mismatch, uint32_t gap, uint32_t end_bonus, uint32_t min_aln_score, uint64_t** map_off_out,
                        awry_map_clip_t** maps_out, awry_pos_t** pos_out, uint64_t** cigar_off_out, uint32_t** cigar_out, uint8_t** status_out) {
  return guarded([&] {
    const Reads q = checked_reads(idx, qbytes, qoff, n, map_off_out);
    const Seeding sc(min_len, max_hits, max_seeds, lookback, max_gap, max_skew, min_score);
    require_map_args(chains_per_strand, max_report, band);
    const AlignMode md = clip_mode(match, mismatch, gap, end_bonus);
    require_cigar_pair(cigar_off_out, cigar_out);
    map_batch(idx, q, sc, (uint32_t)chains_per_strand, (uint32_t)max_report, band, md, clip_map_mode(md, min_aln_score),
              MapOut<awry_map_clip_t>{map_off_out, maps_out, pos_out, cigar_off_out, cigar_out, status_out});
  });
}

int awry_map_split_batch(awry_index_t* idx, const uint8_t* qbytes, const uint64_t* qoff, uint64_t n, uint32_t min_len, uint64_t max_hits, uint32_t max_seeds,
                         uint32_t lookback, uint32_t max_gap, uint32_t max_skew, uint32_t min_score, uint64_t chains_per_strand, uint64_t max_segments,
                         uint64_t max_secondary, uint32_t max_overlap, uint32_t band, uint32_t match, uint32_t mismatch, uint32_t gap, uint32_t end_bonus,
                         uint32_t min_aln_score, uint64_t** map_off_out, awry_map_split_t** maps_out, awry_pos_t** pos_out, uint64_t** cigar_off_out,
                         uint32_t** cigar_out, uint8_t** status_out) {
  return guarded([&] {
    const Reads q = checked_reads(idx, qbytes, qoff, n, map_off_out);
    const Seeding sc(min_len, max_hits, max_seeds, lookback, max_gap, max_skew, min_score);
    const SplitParams sp = split_params(chains_per_strand, max_segments, max_secondary, max_overlap, band);
    const AlignMode md = clip_mode(match, mismatch, gap, end_bonus);
    require_cigar_pair(cigar_off_out, cigar_out);
    split_batch(idx, q, sc, (uint32_t)chains_per_strand, sp, band, md, clip_map_mode(md, min_aln_score),
                MapOut<awry_map_split_t>{map_off_out, maps_out, pos_out, cigar_off_out, cigar_out, status_out});
  });
}

int awry_map_pairs_batch(awry_index_t* idx, const uint8_t* qbytes, const uint64_t* qoff, uint64_t n, uint32_t min_len, uint64_t max_hits, uint32_t max_seeds,
                         uint32_t lookback, uint32_t max_gap, uint32_t max_skew, uint32_t min_score, uint64_t chains_per_strand, uint32_t band,
                         uint64_t min_insert, uint64_t max_insert, uint32_t unpaired_penalty, uint32_t rescue_anchors, int rescue_edits,
                         uint64_t** map_off_out, awry_map_t** maps_out, awry_pos_t** pos_out, uint64_t** cigar_off_out, uint32_t** cigar_out,
                         uint8_t** status_out, uint32_t** insert_out) {
  return guarded([&] {
    const Reads q = checked_reads(idx, qbytes, qoff, n, map_off_out);
    const Seeding sc(min_len, max_hits, max_seeds, lookback, max_gap, max_skew, min_score);
    require_map_args(chains_per_strand, 1, band);
    const PairParams pp = pair_params(min_insert, max_insert, unpaired_penalty, rescue_anchors, rescue_edits);
    require_cigar_pair(cigar_off_out, cigar_out);
    map_pairs_batch(idx, q, sc, (uint32_t)chains_per_strand, band, AlignMode{}, MapMode{}, PairMode{}, pp,
                    MapOut<awry_map_t>{map_off_out, maps_out, pos_out, cigar_off_out, cigar_out, status_out, insert_out});
  });
}

int awry_map_pairs_clip_batch(awry_index_t* idx, const uint8_t* qbytes, const uint64_t* qoff, uint64_t n, uint32_t min_len, uint64_t max_hits,
                              uint32_t max_seeds, uint32_t lookback, uint32_t max_gap, uint32_t max_skew, uint32_t min_score, uint64_t chains_per_strand,
                              uint32_t band, uint64_t min_insert, uint64_t max_insert, uint32_t unpaired_penalty, uint32_t rescue_anchors, int rescue_edits,
                              uint32_t match, uint32_t mismatch, uint32_t gap, uint32_t end_bonus, uint32_t min_aln_score, uint64_t** map_off_out,
                              awry_map_clip_t** maps_out, awry_pos_t** pos_out, uint64_t** cigar_off_out, uint32_t** cigar_out, uint8_t** status_out,
                              uint32_t** insert_out) {
  return guarded([&] {
    const Reads q = checked_reads(idx, qbytes, qoff, n, map_off_out);
    const Seeding sc(min_len, max_hits, max_seeds, lookback, max_gap, max_skew, min_score);
    require_map_args(chains_per_strand, 1, band);
    const PairParams pp = pair_params(min_insert, max_insert, unpaired_penalty, rescue_anchors, rescue_edits, true);
    const AlignMode md = clip_mode(match, mismatch, gap, end_bonus);
    const MapMode mm = clip_map_mode(md, min_aln_score);
    require_cigar_pair(cigar_off_out, cigar_out);
    map_pairs_batch(idx, q, sc, (uint32_t)chains_per_strand, band, md, mm, clip_pair_mode(md, mm), pp,
                    MapOut<awry_map_clip_t>{map_off_out, maps_out, pos_out, cigar_off_out, cigar_out, status_out, insert_out});
  });
}

int awry_locate_edit_batch(awry_index_t* idx, const uint8_t* qbytes, const uint64_t* qoff, uint64_t n, int max_edits, uint64_t max_candidates,
                           uint64_t** hit_off_out, awry_pos_t** hits_out, uint64_t** global_pos_out, uint8_t** edits_out, uint8_t** status_out) {
  return guarded([&] {
    checked_reads(idx, qbytes, qoff, n, hit_off_out);
    require_edits(max_edits);
    require(max_candidates != 0, "max_candidates must be at least 1 (a cap is mandatory: the pieces of a read from a repeat family occur everywhere)");
    locate_edit_batch(idx, qbytes, qoff, n, max_edits, max_candidates, hit_off_out, hits_out, global_pos_out, edits_out, status_out);
  });
}

int awry_align_edit_batch(awry_index_t* idx, const uint8_t* qbytes, const uint64_t* qoff, uint64_t n, int max_edits, uint64_t max_candidates,
                          uint64_t** hit_off_out, awry_pos_t** hits_out, uint64_t** global_pos_out, uint8_t** edits_out, uint8_t** status_out,
                          uint32_t** text_len_out, uint64_t** cigar_off_out, uint32_t** cigar_out) {
  return guarded([&] {
    checked_reads(idx, qbytes, qoff, n, hit_off_out);
    require_edits(max_edits);
    require(max_candidates != 0, "max_candidates must be at least 1 (a cap is mandatory: the pieces of a read from a repeat family occur everywhere)");
    require_cigar_pair(cigar_off_out, cigar_out);
    locate_edit_batch(idx, qbytes, qoff, n, max_edits, max_candidates, hit_off_out, hits_out, global_pos_out, edits_out, status_out, text_len_out,
                      cigar_off_out, cigar_out);
  });
}

namespace {
// one query through the replica's pinned mailbox; want_rows: the range must be a row interval (no text shortcut)
// (the caller holds r.mailbox_mu)
void single_query(Replica& r, const uint8_t* q, uint64_t len, bool want_rows, uint64_t& count, uint64_t& start, uint64_t& end, int ref_kmer_len = -1) {
  Replica::Mailbox& m = r.mailbox;
  if (!m.q) {
    HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&m.q), Replica::Mailbox::QCAP + 16, hipHostMallocDefault));
    HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&m.words), 8 * 8, hipHostMallocDefault));
    HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&m.gpos), Replica::Mailbox::HCAP * 8, hipHostMallocDefault));
    HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&m.pos), Replica::Mailbox::HCAP * 16, hipHostMallocDefault));
  }
  if (len) memcpy(m.q, q, len);
  m.words[0] = 0;
  m.words[1] = len;
  uint8_t* status = reinterpret_cast<uint8_t*>(m.words + 5);
  launch_count_ascii(r, m.q, m.words, 1, m.words + 2, m.words + 3, status, r.stream, !want_rows, 0, want_rows ? ref_kmer_len : -1);
  HIP_CHECK(hipStreamSynchronize(r.stream));
  if (*status != Q_OK) raise_bad_query(0, *status);
  count = m.words[2];
  start = m.words[3];
  end = m.words[4];
}
}  // namespace

int awry_count(awry_index_t* idx, const uint8_t* q, uint64_t len, uint64_t* count) {
  if (idx && count && idx->reps.size() == 1 && (q || len == 0) && len <= Replica::Mailbox::QCAP)
    return guarded([&] {
      uint64_t a = 0, b = 0;
      Replica& r = replica(idx, 0);
      std::lock_guard<std::mutex> lock(r.mailbox_mu);
      single_query(r, q, len, false, *count, a, b);
    });
  const uint64_t off[2] = {0, len};
  return awry_count_batch(idx, q, off, 1, count);
}

int awry_search_range(awry_index_t* idx, const uint8_t* q, uint64_t len, awry_range_t* out) {
  return guarded([&] {
    require(idx && out && (q || len == 0), "null argument");
    Replica& r = replica(idx, 0);
    if (len <= Replica::Mailbox::QCAP) {
      uint64_t c = 0;
      std::lock_guard<std::mutex> lock(r.mailbox_mu);
      single_query(r, q, len, true, c, out->start_ptr, out->end_ptr, (int)idx->host.kmer_len);
      return;
    }
    ChunkBuffers cb;
    const uint64_t off[2] = {0, len};
    run_count_chunk(r, cb, q, off, Shard{0, 1}, true, false, (int)idx->host.kmer_len);  // the caller wants rows: the reference's schedule
    uint64_t h[2];
    HIP_CHECK(hipMemcpyAsync(h, cb.ranges.p, 16, hipMemcpyDeviceToHost, r.stream));
    HIP_CHECK(hipStreamSynchronize(r.stream));
    check_status(cb, 0);
    out->start_ptr = h[0];
    out->end_ptr = h[1];
  });
}

int awry_locate(awry_index_t* idx, const uint8_t* q, uint64_t len, awry_pos_t** hits_out, uint64_t** global_pos_out,
                uint64_t* n_hits) {
  if (idx && hits_out && idx->reps.size() == 1 && (q || len == 0) && len <= Replica::Mailbox::QCAP) {
    // one query: count through the mailbox, then -- for a hit list that fits it -- locate straight into pinned memory
    bool done = false;
    int rc = guarded([&] {
      Replica& r = replica(idx, 0);
      std::lock_guard<std::mutex> lock(r.mailbox_mu);
      uint64_t count = 0, rs = 0, unused = 0;
      single_query(r, q, len, false, count, rs, unused);
      if (count > Replica::Mailbox::HCAP) return;  // the batch path sizes its own buffers
      Replica::Mailbox& m = r.mailbox;
      std::unique_ptr<awry_pos_t, decltype(&free)> hits(malloc_array<awry_pos_t>(count), &free);
      std::unique_ptr<uint64_t, decltype(&free)> gp(global_pos_out ? malloc_array<uint64_t>(count) : nullptr, &free);
      if (count) {
        m.words[6] = 0;
        m.words[7] = count;
        launch_locate(r, m.words + 3, 2, m.words + 6, 1, count, m.gpos, m.pos, r.stream);
        HIP_CHECK(hipStreamSynchronize(r.stream));
        memcpy(hits.get(), m.pos, count * sizeof(awry_pos_t));
        if (gp) memcpy(gp.get(), m.gpos, count * 8);
      }
      *hits_out = hits.release();
      if (global_pos_out) *global_pos_out = gp.release();
      if (n_hits) *n_hits = count;
      done = true;
    });
    if (rc != AWRY_OK || done) return rc;
  }
  const uint64_t off[2] = {0, len};
  uint64_t* hit_off = nullptr;
  int rc = awry_locate_batch(idx, q, off, 1, &hit_off, hits_out, global_pos_out);
  if (rc == AWRY_OK) {
    if (n_hits) *n_hits = hit_off[1];
    release_result(hit_off);
  }
  return rc;
}

int awry_initial_range(const awry_index_t* idx, uint8_t symbol_ascii, awry_range_t* out) {
  return guarded([&] {
    require(idx && out, "null argument");
    int s = checked_symbol(idx, symbol_ascii);
    out->start_ptr = idx->host.prefix_sums[s];           // src/search.rs:43-48
    out->end_ptr = idx->host.prefix_sums[s + 1] - 1;
  });
}

int awry_update_range(awry_index_t* idx, awry_range_t in, uint8_t symbol_ascii, awry_range_t* out) {
  return guarded([&] {
    require(idx && out, "null argument");
    int s = checked_symbol(idx, symbol_ascii);
    if (s == 0) throw QueryError("cannot extend a range with the sentinel (src/bwt.rs:126-128 panics)");
    if (in.start_ptr == 0 || in.start_ptr > idx->host.bwt_len || in.end_ptr >= idx->host.bwt_len)
      throw ArgError("range outside the BWT");
    out->start_ptr = scalar_op(idx, 0, in.start_ptr, in.end_ptr, s, &out->end_ptr);
  });
}

int awry_backstep(awry_index_t* idx, uint64_t row, uint64_t* out) {
  return guarded([&] {
    require(idx && out, "null argument");
    require(row < idx->host.bwt_len, "row outside the BWT");
    *out = scalar_op(idx, 1, row, 0, 0);
  });
}

int awry_get_seq_location(const awry_index_t* idx, uint64_t g, awry_pos_t* out) {
  return guarded([&] {
    require(idx && out, "null argument");
    const auto& st = idx->host.seq_starts;
    require(!st.empty(), "index has no sequence records");
    size_t i = (size_t)(std::upper_bound(st.begin(), st.end(), g) - st.begin());
    i = i ? i - 1 : 0;
    out->seq_idx = i;
    out->local_pos = g - st[i];
  });
}

int awry_alphabet(const awry_index_t* idx) { return idx ? idx->host.alphabet : -1; }
uint64_t awry_bwt_len(const awry_index_t* idx) { return idx ? idx->host.bwt_len : 0; }
uint64_t awry_version(const awry_index_t* idx) { return idx ? idx->host.version : 0; }
uint64_t awry_sa_ratio(const awry_index_t* idx) { return idx ? idx->host.sa_ratio : 0; }
uint8_t awry_kmer_len(const awry_index_t* idx) { return idx ? idx->host.kmer_len : 0; }
uint64_t awry_sentinel_row(const awry_index_t* idx) { return idx ? idx->host.sentinel_row : 0; }
const uint64_t* awry_prefix_sums(const awry_index_t* idx, uint64_t* len) {
  if (!idx) return nullptr;
  if (len) *len = idx->host.prefix_sums.size();
  return idx->host.prefix_sums.data();
}
uint64_t awry_num_sequences(const awry_index_t* idx) { return idx ? idx->host.seq_starts.size() : 0; }
uint64_t awry_sequence_start(const awry_index_t* idx, uint64_t i) {
  return idx && i < idx->host.seq_starts.size() ? idx->host.seq_starts[i] : 0;
}
const char* awry_sequence_header(const awry_index_t* idx, uint64_t i) {
  return idx && i < idx->host.headers.size() ? idx->host.headers[i].c_str() : nullptr;
}
const uint64_t* awry_block_words(const awry_index_t* idx, uint64_t* nwords) {
  if (!idx) return nullptr;
  if (nwords) *nwords = idx->host.blocks.size();
  return idx->host.blocks.data();
}
const uint64_t* awry_sa_words(const awry_index_t* idx, uint64_t* nwords) {
  if (!idx) return nullptr;
  if (nwords) *nwords = idx->host.sa_words.size();
  return idx->host.sa_words.data();
}
int awry_block_reference_layout(const awry_index_t* idx, uint64_t block, uint64_t* out, uint64_t out_words) {
  return guarded([&] {
    require(idx && out, "null argument");
    require(block < idx->host.nblocks, "block out of range");
    const uint64_t need = 4 * num_planes(idx->host.alphabet) + (idx->host.alphabet == NUCLEOTIDE ? 8 : 24);
    require(out_words >= need, "output buffer too small");
    block_to_reference(idx->host, block, out);
  });
}

int awry_read_query_file(const char* path, uint8_t** qbytes_out, uint64_t** qoff_out, uint64_t* n_out) {
  return guarded([&] {
    require(path && qbytes_out && qoff_out && n_out, "null argument");
    read_query_file(path, qbytes_out, qoff_out, n_out);
  });
}

int awry_host_suffix_array(const uint8_t* text, uint64_t n, uint64_t* sa_out) {
  return guarded([&] {
    require(text && sa_out, "null argument");
    suffix_array_bytes(text, n, sa_out);
  });
}
uint8_t awry_symbol_index(int alphabet, uint8_t ascii) { return (uint8_t)index_of_ascii(alphabet, ascii); }

int awry_host_pack_nt2(const uint8_t* qbytes, const uint64_t* qoff, uint64_t n, uint64_t L, uint64_t* words_out, uint32_t* lens_out,
                       uint32_t* bad_out, uint64_t* nbad_out) {
  return guarded([&] {
    require((qbytes && words_out && nbad_out) || n == 0, "null argument");
    require(L >= 1 && L <= 4096, "packed query length out of range");
    if (nbad_out) *nbad_out = 0;
    if (n == 0) return;
    if (qoff)
      for (uint64_t i = 0; i < n; i++) require(qoff[i + 1] >= qoff[i] && qoff[i + 1] - qoff[i] >= 1 && qoff[i + 1] - qoff[i] <= L, "query length outside 1..L");
    std::vector<uint32_t> bad;
    const uint8_t* first = qbytes + (qoff ? qoff[0] : 0);
    pack_nt2_host(first, qbytes + (qoff ? qoff[n] : n * L), qoff, 0, n, L, words_out, qoff ? lens_out : nullptr, bad);
    *nbad_out = bad.size();
    if (bad_out) std::copy(bad.begin(), bad.end(), bad_out);
  });
}
int awry_host_threads(void) { return (int)HostPool::instance().threads(); }
void awry_host_memcpy(void* dst, const void* src, uint64_t bytes) { pool_memcpy(dst, src, bytes); }

// ---- device-resident API -----------------------------------------------------------------------------

int awry_dev_pack_nt2(awry_index_t* idx, int slot, const void* d_ascii, uint64_t n, int L, void* d_words, void* d_bad, void* stream) {
  return guarded([&] {
    Replica& r = replica(idx, slot);
    require(L >= 1 && L <= (1 << 20), "packed read length out of range");
    require(d_ascii && d_words && d_bad, "null device pointer");
    if (n == 0) return;
    launch_pack_nt2(r, (const uint8_t*)d_ascii, nullptr, 0, n, n * (uint64_t)L, L, (L + 31) / 32, (uint64_t*)d_words, nullptr,
                    (unsigned long long*)d_bad, (hipStream_t)stream);
  });
}

int awry_dev_count_nt2(awry_index_t* idx, int slot, const void* d_words, uint64_t n, int L, void* d_counts, int use_seed, void* stream) {
  return guarded([&] {
    Replica& r = replica(idx, slot);
    require((d_words && d_counts) || n == 0, "null device pointer");
    launch_count_nt2(r, (const uint64_t*)d_words, n, L, (uint64_t*)d_counts, use_seed != 0, (hipStream_t)stream);
  });
}

int awry_dev_count_nt2_tally(awry_index_t* idx, int slot, const void* d_words, uint64_t n, int L, void* d_counts, int use_seed,
                             void* d_tally, void* stream) {
  return guarded([&] {
    Replica& r = replica(idx, slot);
    require((d_words && d_counts && d_tally) || n == 0, "null device pointer");
    launch_count_nt2(r, (const uint64_t*)d_words, n, L, (uint64_t*)d_counts, use_seed != 0, (hipStream_t)stream,
                     (unsigned long long*)d_tally);
  });
}

int awry_dev_count_nt2_long(awry_index_t* idx, int slot, const void* d_words, uint64_t n, int L, void* d_counts, void* d_range_start,
                            int use_seed, void* stream) {
  return guarded([&] {
    Replica& r = replica(idx, slot);
    require((d_words && d_counts) || n == 0, "null device pointer");
    launch_count_nt2_long(r, (const uint64_t*)d_words, n, L, (uint64_t*)d_counts, (uint64_t*)d_range_start, use_seed != 0, (hipStream_t)stream);
  });
}

int awry_set_locate_sa_ratio(awry_index_t* idx, int ratio) {
  return guarded([&] {
    require(idx != nullptr, "null index");
    require(ratio >= 0 && ratio <= 1024, "dense SA ratio must be in 0..1024");
    idx->dense_ratio_request = ratio;
    change_replicas(idx, [&](Replica& r) { rebuild_dense_sa(idx, r, ratio); });
  });
}
int awry_set_verify(awry_index_t* idx, int after_steps) {
  return guarded([&] {
    require(idx != nullptr, "null index");
    require(after_steps >= -1 && after_steps <= 1000, "verify threshold out of range");
    idx->verify_request = after_steps;
    if (after_steps >= 0) idx->dense_ratio_request = 1;
    change_replicas(idx, [&](Replica& r) { rebuild_verify(idx, r, after_steps); });
  });
}
int awry_set_verify_kmers(awry_index_t* idx, int on) {
  return guarded([&] {
    require(idx != nullptr, "null index");
    idx->verify_kmers_request = on != 0;
    for (auto& r : idx->reps) r->verify_kmers = on != 0;
  });
}
int awry_set_lcx(awry_index_t* idx, int on) {
  return guarded([&] {
    require(idx != nullptr, "null index");
    idx->lcx_request = on ? -1 : 0;
    change_replicas(idx, [](Replica&) {});
  });
}
int awry_lcx_enabled(const awry_index_t* idx) { return idx && !idx->reps.empty() && idx->reps[0]->lcx_key.p != nullptr; }
int awry_set_kmer_table(awry_index_t* idx, int mode) {
  return guarded([&] {
    require(idx != nullptr, "null index");
    require(mode >= -1 && mode <= 1, "k-mer table mode must be -1 (policy), 0 (off) or 1 (build for the next length)");
    idx->kmer_table_request = mode;
    for (size_t s = 0; s < idx->reps.size(); s++) {
      Replica& r = replica(idx, (int)s);
      r.kt_mode = mode;
      if (mode == 0) drop_kmer_table(r);
    }
  });
}
int awry_kmer_table_info(awry_index_t* idx, int slot, uint64_t* info) {
  return guarded([&] {
    require(idx != nullptr && info != nullptr, "null argument");
    Replica& r = replica(idx, slot);
    std::shared_lock<std::shared_mutex> lock(r.kt_mu);
    const bool have = r.kt.tab.p != nullptr;
    info[0] = have ? (uint64_t)r.kt.L : 0;
    info[1] = r.kt.entries;
    info[2] = have ? 1ull << r.kt.bits : 0;
    info[3] = r.kt.overflowed;
    info[4] = have ? 128ull << r.kt.bits : 0;
    info[5] = (uint64_t)(r.kt.build_ms * 1000.0);
  });
}
int awry_debug_set_kmer_table_lines(uint64_t lines) { g_kt_debug_lines.store(lines); return AWRY_OK; }
int awry_debug_kmer_table(awry_index_t* idx, int slot, uint64_t* host_out, uint64_t capacity_words, int* L_out, uint32_t* bits_out) {
  return guarded([&] {
    require(idx != nullptr && L_out != nullptr && bits_out != nullptr, "null argument");
    Replica& r = replica(idx, slot);
    std::shared_lock<std::shared_mutex> lock(r.kt_mu);  // (held over the copy: a launch of another length frees the table)
    const bool have = r.kt.tab.p != nullptr;
    *L_out = have ? r.kt.L : 0;
    *bits_out = have ? r.kt.bits : 0u;
    if (!have || !host_out || capacity_words < (16ull << r.kt.bits)) return;
    HIP_CHECK(hipMemcpyAsync(host_out, r.kt.tab.p, 128ull << r.kt.bits, hipMemcpyDeviceToHost, r.stream));
    HIP_CHECK(hipStreamSynchronize(r.stream));
  });
}
int awry_debug_lcx(const awry_index_t* idx, int slot, const void** d_keys, const void** d_rowpos) {
  if (!idx || slot < 0 || slot >= (int)idx->reps.size() || !d_keys || !d_rowpos) return AWRY_ERR_ARG;
  *d_keys = idx->reps[slot]->lcx_key.p;
  *d_rowpos = idx->reps[slot]->lcx_rowpos.p;
  return AWRY_OK;
}
const void* awry_debug_dense_sa(const awry_index_t* idx, int slot) {
  return idx && slot >= 0 && slot < (int)idx->reps.size() ? (const void*)idx->reps[slot]->dense_sa.p : nullptr;
}
int awry_debug_accelerators(const awry_index_t* idx, int slot, awry_debug_accel_t* out) {
  if (!idx || slot < 0 || slot >= (int)idx->reps.size() || !out) return AWRY_ERR_ARG;
  const Replica& r = *idx->reps[slot];
  *out = awry_debug_accel_t{};
  out->seed = r.wide ? (const void*)r.seed64.p : (const void*)r.seed.p;
  out->seed_k = out->seed ? r.seed_k : 0;
  out->seed_entry_bytes = r.wide ? (int32_t)sizeof(SeedEntry64) : (int32_t)sizeof(SeedEntry);
  out->seed_pos = r.seed_pos ? 1 : 0;
  out->ctx_extra = r.ctx_extra;
  out->dense_sa = r.dense_sa.p;
  out->dense_ratio = r.dense_ratio;
  out->text4 = r.text4.p;
  out->text4_words = r.text4.p ? r.text4.n : 0;
  out->text8 = r.text8.p;
  out->sa_nblock = r.sa_nblock.p;
  if (r.sa_nblock.p) {
    out->nblock_lo = idx->host.prefix_sums[4];
    out->nblock_hi = idx->host.prefix_sums[5];
  }
  out->lcx_inner = r.lcx_inner.p;
  out->lcx_inner_words = r.lcx_inner.p ? r.lcx_inner.n : 0;
  for (int t = 0; t < 8; t++) out->lcx_off[t] = r.lcx_off[t];
  return AWRY_OK;
}
const void* awry_debug_seed_rung(awry_index_t* idx, int slot, int L) {
  const void* p = nullptr;
  (void)guarded([&] { p = seed_rung(replica(idx, slot), L); });
  return p;
}
int awry_debug_set_ctx_extra_cap(int cap) {
  if (cap < -1) { g_last_error = "awry_debug_set_ctx_extra_cap: a cap below -1"; return AWRY_ERR_ARG; }
  g_ctx_extra_cap.store(cap);
  return AWRY_OK;
}
int awry_verify_enabled(const awry_index_t* idx) {
  return idx && !idx->reps.empty() && (idx->reps[0]->text4.p != nullptr || idx->reps[0]->text8.p != nullptr);
}

int awry_locate_sa_ratio(const awry_index_t* idx) {
  if (!idx || idx->reps.empty()) return 0;
  return idx->reps[0]->dense_ratio ? (int)idx->reps[0]->dense_ratio : (int)idx->host.sa_ratio;
}

int awry_dev_count_ascii(awry_index_t* idx, int slot, const void* d_qbytes, const void* d_qoff, uint64_t n, void* d_counts,
                         void* d_ranges, void* d_status, void* stream) {
  return guarded([&] {
    Replica& r = replica(idx, slot);
    require((d_qoff && d_counts) || n == 0, "null device pointer");
    launch_count_ascii(r, (const uint8_t*)d_qbytes, (const uint64_t*)d_qoff, n, (uint64_t*)d_counts, (uint64_t*)d_ranges,
                       (uint8_t*)d_status, (hipStream_t)stream, d_ranges == nullptr);  // ranges requested: they are row intervals
  });
}

int awry_dev_count_ascii_for_locate(awry_index_t* idx, int slot, const void* d_qbytes, const void* d_qoff, uint64_t n, void* d_counts,
                                    void* d_locate_words, void* d_status, void* stream) {
  return guarded([&] {
    Replica& r = replica(idx, slot);
    require((d_qoff && d_counts && d_locate_words) || n == 0, "null device pointer");
    launch_count_ascii(r, (const uint8_t*)d_qbytes, (const uint64_t*)d_qoff, n, (uint64_t*)d_counts, (uint64_t*)d_locate_words,
                       (uint8_t*)d_status, (hipStream_t)stream, true);  // RS_* words where the count pass verified against the text
  });
}

int awry_dev_count_ascii_uniform(awry_index_t* idx, int slot, const void* d_qbytes, uint64_t n, uint64_t len, void* d_counts,
                                 void* d_status, void* stream) {
  return guarded([&] {
    Replica& r = replica(idx, slot);
    require((d_qbytes && d_counts) || n == 0, "null device pointer");
    launch_count_ascii_uniform(r, (const uint8_t*)d_qbytes, n, len, (uint64_t*)d_counts, (uint8_t*)d_status, (hipStream_t)stream);
  });
}

int awry_dev_count_ascii_uniform_tally(awry_index_t* idx, int slot, const void* d_qbytes, uint64_t n, uint64_t len, void* d_counts,
                                       void* d_tally, void* stream) {
  return guarded([&] {
    Replica& r = replica(idx, slot);
    require((d_qbytes && d_counts && d_tally) || n == 0, "null device pointer");
    require(r.dev.alphabet == AMINO, "the census of the uniform entry point is kept by the amino k-mer schedule");
    launch_count_ascii_uniform(r, (const uint8_t*)d_qbytes, n, len, (uint64_t*)d_counts, nullptr, (hipStream_t)stream, nullptr,
                               (unsigned long long*)d_tally);
  });
}

uint64_t awry_dev_scan_scratch_bytes(uint64_t n) { return (scan_tiles(n) + 1) * 8; }

int awry_dev_scan_counts(awry_index_t* idx, int slot, const void* d_counts, uint64_t n, void* d_hit_off, void* d_scratch, void* stream) {
  return guarded([&] {
    Replica& r = replica(idx, slot);
    require(d_hit_off && ((d_counts && d_scratch) || n == 0), "null device pointer");
    launch_scan(r, (const uint64_t*)d_counts, n, (uint64_t*)d_hit_off, (uint64_t*)d_scratch, (hipStream_t)stream);
  });
}

int awry_dev_locate(awry_index_t* idx, int slot, const void* d_ranges, int range_stride, const void* d_hit_off, uint64_t n,
                    uint64_t total, void* d_global_pos, void* d_pos, void* stream) {
  return guarded([&] {
    Replica& r = replica(idx, slot);
    require((d_ranges && d_hit_off && d_global_pos) || total == 0, "null device pointer");
    require(range_stride == 1 || range_stride == 2, "range_stride must be 1 (starts) or 2 ((start,end) pairs)");
    launch_locate(r, (const uint64_t*)d_ranges, range_stride, (const uint64_t*)d_hit_off, n, total, (uint64_t*)d_global_pos,
                  (uint64_t*)d_pos, (hipStream_t)stream);
  });
}

int awry_dev_locate_tally(awry_index_t* idx, int slot, const void* d_ranges, int range_stride, const void* d_hit_off, uint64_t n,
                          uint64_t total, void* d_global_pos, void* d_pos, void* d_tally, void* stream) {
  return guarded([&] {
    Replica& r = replica(idx, slot);
    require((d_ranges && d_hit_off && d_global_pos && d_tally) || total == 0, "null device pointer");
    require(range_stride == 1 || range_stride == 2, "range_stride must be 1 (starts) or 2 ((start,end) pairs)");
    require(r.dev.alphabet == NUCLEOTIDE, "the walk census is kept by the nucleotide walk kernel");
    launch_locate(r, (const uint64_t*)d_ranges, range_stride, (const uint64_t*)d_hit_off, n, total, (uint64_t*)d_global_pos,
                  (uint64_t*)d_pos, (hipStream_t)stream, (unsigned long long*)d_tally);
  });
}

int awry_dev_count_mismatch(awry_index_t* idx, int slot, const void* d_qbytes, const void* d_qoff, uint64_t n, int max_mismatches,
                            void* d_counts, void* d_status, void* stream) {
  return awry_dev_count_mismatch_tally(idx, slot, d_qbytes, d_qoff, n, max_mismatches, d_counts, d_status, nullptr, stream);
}

int awry_dev_count_mismatch_tally(awry_index_t* idx, int slot, const void* d_qbytes, const void* d_qoff, uint64_t n, int max_mismatches,
                                  void* d_counts, void* d_status, void* d_tally, void* stream) {
  return guarded([&] { dev_count_leaves(idx, slot, false, d_qbytes, d_qoff, n, max_mismatches, d_counts, d_status, d_tally, stream); });
}

int awry_dev_count_pattern(awry_index_t* idx, int slot, const void* d_qbytes, const void* d_qoff, uint64_t n, int max_mismatches,
                           void* d_counts, void* d_status, void* stream) {
  return awry_dev_count_pattern_tally(idx, slot, d_qbytes, d_qoff, n, max_mismatches, d_counts, d_status, nullptr, stream);
}

int awry_dev_count_pattern_tally(awry_index_t* idx, int slot, const void* d_qbytes, const void* d_qoff, uint64_t n, int max_mismatches,
                                 void* d_counts, void* d_status, void* d_tally, void* stream) {
  return guarded([&] { dev_count_leaves(idx, slot, true, d_qbytes, d_qoff, n, max_mismatches, d_counts, d_status, d_tally, stream); });
}

int awry_dev_anchors(awry_index_t* idx, int slot, const void* d_qbytes, const void* d_qoff, uint64_t n, uint32_t min_len, int skip,
                     void* d_n_anchors, const void* d_anchor_off, void* d_anchors, void* d_status, void* stream) {
  return awry_dev_anchors_tally(idx, slot, d_qbytes, d_qoff, n, min_len, skip, d_n_anchors, d_anchor_off, d_anchors, d_status, nullptr, stream);
}

int awry_dev_anchors_tally(awry_index_t* idx, int slot, const void* d_qbytes, const void* d_qoff, uint64_t n, uint32_t min_len, int skip,
                           void* d_n_anchors, const void* d_anchor_off, void* d_anchors, void* d_status, void* d_tally, void* stream) {
  return guarded([&] {
    require_anchor_args(min_len, skip);
    Replica& r = replica(idx, slot);
    require(n == 0 || (d_qbytes && d_qoff && (d_anchor_off ? d_anchors != nullptr : d_n_anchors != nullptr)), "null device pointer");
    launch_anchors(r, (const uint8_t*)d_qbytes, (const uint64_t*)d_qoff, n, min_len, skip, (uint64_t*)d_n_anchors, (const uint64_t*)d_anchor_off,
                   (Anchor*)d_anchors, (uint8_t*)d_status, (hipStream_t)stream, (unsigned long long*)d_tally);
  });
}

int awry_dev_smems(awry_index_t* idx, int slot, const void* d_qbytes, const void* d_qoff, uint64_t n, uint32_t min_len, void* d_n_smems,
                   const void* d_smem_off, void* d_smems, void* d_status, void* stream) {
  return awry_dev_smems_tally(idx, slot, d_qbytes, d_qoff, n, min_len, d_n_smems, d_smem_off, d_smems, d_status, nullptr, stream);
}

int awry_dev_smems_tally(awry_index_t* idx, int slot, const void* d_qbytes, const void* d_qoff, uint64_t n, uint32_t min_len, void* d_n_smems,
                         const void* d_smem_off, void* d_smems, void* d_status, void* d_tally, void* stream) {
  return guarded([&] {
    require_smem_args(min_len);
    Replica& r = replica(idx, slot);
    require(n == 0 || (d_qbytes && d_qoff && (d_smem_off ? d_smems != nullptr : d_n_smems != nullptr)), "null device pointer");
    launch_smems(r, (const uint8_t*)d_qbytes, (const uint64_t*)d_qoff, n, min_len, (uint64_t*)d_n_smems, (const uint64_t*)d_smem_off, (Anchor*)d_smems,
                 (uint8_t*)d_status, (hipStream_t)stream, (unsigned long long*)d_tally);
  });
}

int awry_dev_edit_windows(awry_index_t* idx, int slot, const uint8_t* d_qbytes, const uint64_t* d_qoff, const uint32_t* d_win_query,
                          const uint64_t* d_win_first, const uint32_t* d_win_count, uint64_t m, int max_edits, uint64_t* d_n_hits, const uint64_t* d_hit_off,
                          uint64_t* d_gpos, uint8_t* d_edits, void* stream) {
  return awry_dev_edit_windows_tally(idx, slot, d_qbytes, d_qoff, d_win_query, d_win_first, d_win_count, m, max_edits, d_n_hits, d_hit_off, d_gpos, d_edits,
                                     nullptr, stream);
}

int awry_dev_edit_windows_tally(awry_index_t* idx, int slot, const uint8_t* d_qbytes, const uint64_t* d_qoff, const uint32_t* d_win_query,
                                const uint64_t* d_win_first, const uint32_t* d_win_count, uint64_t m, int max_edits, uint64_t* d_n_hits,
                                const uint64_t* d_hit_off, uint64_t* d_gpos, uint8_t* d_edits, uint64_t* d_tally, void* stream) {
  return guarded([&] {
    require_edits(max_edits);
    Replica& r = replica(idx, slot);
    require(m == 0 || (d_qbytes && d_qoff && d_win_query && d_win_first && d_win_count && (d_hit_off ? d_gpos && d_edits : d_n_hits != nullptr)),
            "null device pointer");
    launch_edit_windows(r, edit_text(r), d_qbytes, d_qoff, d_win_query, d_win_first, d_win_count, m, max_edits, EDIT_MAX_W, 0, d_n_hits, d_hit_off, d_gpos,
                        d_edits, (hipStream_t)stream, (unsigned long long*)d_tally);
  });
}

int awry_dev_edit_align(awry_index_t* idx, int slot, const uint8_t* d_qbytes, const uint64_t* d_qoff, const uint32_t* d_hit_query,
                        const uint64_t* d_hit_gpos, const uint8_t* d_hit_edits, uint64_t m, int max_edits, uint32_t* d_text_len, uint8_t* d_n_ops,
                        uint32_t* d_ops, void* stream) {
  return awry_dev_edit_align_tally(idx, slot, d_qbytes, d_qoff, d_hit_query, d_hit_gpos, d_hit_edits, m, max_edits, d_text_len, d_n_ops, d_ops, nullptr,
                                   stream);
}

int awry_dev_edit_align_tally(awry_index_t* idx, int slot, const uint8_t* d_qbytes, const uint64_t* d_qoff, const uint32_t* d_hit_query,
                              const uint64_t* d_hit_gpos, const uint8_t* d_hit_edits, uint64_t m, int max_edits, uint32_t* d_text_len, uint8_t* d_n_ops,
                              uint32_t* d_ops, uint64_t* d_tally, void* stream) {
  return guarded([&] {
    require_edits(max_edits);
    Replica& r = replica(idx, slot);
    require(m == 0 || (d_qbytes && d_qoff && d_hit_query && d_hit_gpos && d_hit_edits && d_text_len && d_n_ops && d_ops), "null device pointer");
    launch_edit_align(r, edit_text(r), d_qbytes, d_qoff, d_hit_query, d_hit_gpos, d_hit_edits, m, max_edits, EDIT_MAX_LEN, d_text_len, d_n_ops, d_ops,
                      (hipStream_t)stream, (unsigned long long*)d_tally);
  });
}

int awry_dev_chain_seeds(awry_index_t* idx, int slot, const uint64_t* d_seed_off, const awry_seed_t* d_seeds, uint64_t n, uint32_t max_seeds,
                         uint32_t lookback, uint32_t max_gap, uint32_t max_skew, uint32_t min_score, uint64_t* d_n_chains, uint64_t* d_n_members,
                         const uint64_t* d_chain_off, const uint64_t* d_member_off, awry_chain_t* d_chains, awry_seed_t* d_members, uint8_t* d_status,
                         void* stream) {
  return awry_dev_chain_seeds_tally(idx, slot, d_seed_off, d_seeds, n, max_seeds, lookback, max_gap, max_skew, min_score, d_n_chains, d_n_members,
                                    d_chain_off, d_member_off, d_chains, d_members, d_status, nullptr, stream);
}

int awry_dev_chain_seeds_tally(awry_index_t* idx, int slot, const uint64_t* d_seed_off, const awry_seed_t* d_seeds, uint64_t n, uint32_t max_seeds,
                               uint32_t lookback, uint32_t max_gap, uint32_t max_skew, uint32_t min_score, uint64_t* d_n_chains, uint64_t* d_n_members,
                               const uint64_t* d_chain_off, const uint64_t* d_member_off, awry_chain_t* d_chains, awry_seed_t* d_members,
                               uint8_t* d_status, uint64_t* d_tally, void* stream) {
  return guarded([&] {
    const ChainParams P = chain_params(max_seeds, lookback, max_gap, max_skew, min_score);
    Replica& r = replica(idx, slot);
    require_chain_index(r.dev.bwt_len);
    require(n == 0 || (d_seed_off && (d_chain_off ? d_member_off && d_chains && d_members : d_n_chains && d_n_members)), "null device pointer");
    launch_chain(r, d_seed_off, reinterpret_cast<const Seed*>(d_seeds), n, P, d_n_chains, d_n_members, d_chain_off, d_member_off,
                 reinterpret_cast<Chain*>(d_chains), reinterpret_cast<Seed*>(d_members), d_status, (hipStream_t)stream, (unsigned long long*)d_tally);
  });
}

int awry_dev_align_chains(awry_index_t* idx, int slot, const uint8_t* d_qbytes, const uint64_t* d_qoff, const uint32_t* d_chain_query,
                          const uint64_t* d_member_off, const awry_seed_t* d_members, uint64_t m, uint32_t band, awry_aln_t* d_alns, uint64_t* d_n_ops,
                          const uint64_t* d_cigar_off, uint32_t* d_cigar, void* stream) {
  return awry_dev_align_chains_tally(idx, slot, d_qbytes, d_qoff, d_chain_query, d_member_off, d_members, m, band, d_alns, d_n_ops, d_cigar_off, d_cigar,
                                     nullptr, stream);
}

int awry_dev_align_chains_tally(awry_index_t* idx, int slot, const uint8_t* d_qbytes, const uint64_t* d_qoff, const uint32_t* d_chain_query,
                                const uint64_t* d_member_off, const awry_seed_t* d_members, uint64_t m, uint32_t band, awry_aln_t* d_alns,
                                uint64_t* d_n_ops, const uint64_t* d_cigar_off, uint32_t* d_cigar, uint64_t* d_tally, void* stream) {
  return guarded([&] {
    require_chain_align_args(1, band);
    Replica& r = replica(idx, slot);
    require(m == 0 || (d_qbytes && d_qoff && d_chain_query && d_member_off && d_members && (d_cigar_off ? d_cigar != nullptr : d_alns && d_n_ops)),
            "null device pointer");
    launch_chain_align(r, edit_text(r), d_qbytes, d_qoff, d_chain_query, d_member_off, reinterpret_cast<const Seed*>(d_members), m, (int)band, AlignMode{},
                       CHAIN_ALIGN_MAX_LEN, d_alns, d_n_ops, d_cigar_off, d_cigar, (hipStream_t)stream, (unsigned long long*)d_tally);
  });
}

int awry_dev_align_chains_clip(awry_index_t* idx, int slot, const uint8_t* d_qbytes, const uint64_t* d_qoff, const uint32_t* d_chain_query,
                               const uint64_t* d_member_off, const awry_seed_t* d_members, uint64_t m, uint32_t band, uint32_t match, uint32_t mismatch,
                               uint32_t gap, uint32_t end_bonus, awry_aln_clip_t* d_alns, uint64_t* d_n_ops, const uint64_t* d_cigar_off, uint32_t* d_cigar,
                               void* stream) {
  return awry_dev_align_chains_clip_tally(idx, slot, d_qbytes, d_qoff, d_chain_query, d_member_off, d_members, m, band, match, mismatch, gap, end_bonus,
                                          d_alns, d_n_ops, d_cigar_off, d_cigar, nullptr, stream);
}

int awry_dev_align_chains_clip_tally(awry_index_t* idx, int slot, const uint8_t* d_qbytes, const uint64_t* d_qoff, const uint32_t* d_chain_query,
                                     const uint64_t* d_member_off, const awry_seed_t* d_members, uint64_t m, uint32_t band, uint32_t match,
                                     uint32_t mismatch, uint32_t gap, uint32_t end_bonus, awry_aln_clip_t* d_alns, uint64_t* d_n_ops,
                                     const uint64_t* d_cigar_off, uint32_t* d_cigar, uint64_t* d_tally, void* stream) {
  return guarded([&] {
    require_chain_align_args(1, band);
    const AlignMode md = clip_mode(match, mismatch, gap, end_bonus);
    Replica& r = replica(idx, slot);
    require(m == 0 || (d_qbytes && d_qoff && d_chain_query && d_member_off && d_members && (d_cigar_off ? d_cigar != nullptr : d_alns && d_n_ops)),
            "null device pointer");
    launch_chain_align(r, edit_text(r), d_qbytes, d_qoff, d_chain_query, d_member_off, reinterpret_cast<const Seed*>(d_members), m, (int)band, md,
                       CHAIN_ALIGN_MAX_LEN, d_alns, d_n_ops, d_cigar_off, d_cigar, (hipStream_t)stream, (unsigned long long*)d_tally);
  });
}

int awry_dev_revcomp(awry_index_t* idx, int slot, const uint8_t* d_qbytes, const uint64_t* d_qoff, uint64_t n, uint8_t* d_out_bytes, uint64_t* d_out_off,
                     void* stream) {
  return guarded([&] {
    require(idx != nullptr, "null argument");
    if (idx->host.alphabet != NUCLEOTIDE) throw ArgError("the reverse complement needs a nucleotide index");
    Replica& r = replica(idx, slot);
    require(d_out_off && (n == 0 || (d_qbytes && d_qoff && d_out_bytes)), "null device pointer");
    launch_strand_expand(r, d_qbytes, d_qoff, n, d_out_bytes, d_out_off, (hipStream_t)stream);
  });
}

int awry_dev_map_select(awry_index_t* idx, int slot, const uint64_t* d_aln_off, const awry_aln_t* d_alns, const awry_chain_t* d_chains,
                        const uint8_t* d_chain_status, uint64_t n, uint32_t chains_per_strand, uint32_t max_report, uint64_t* d_n_maps,
                        uint8_t* d_read_status, const uint64_t* d_map_off, awry_map_t* d_maps, uint32_t* d_sel, awry_pos_t* d_pos, void* stream) {
  return guarded([&] {
    require_map_args(chains_per_strand, max_report, 0);
    Replica& r = replica(idx, slot);
    require(n == 0 || (d_aln_off && d_alns && d_chains && (d_map_off ? d_maps != nullptr : d_n_maps != nullptr)), "null device pointer");
    launch_map_select(r, d_aln_off, d_alns, reinterpret_cast<const Chain*>(d_chains), d_chain_status, n, chains_per_strand, max_report, MapMode{}, d_n_maps,
                      d_read_status, d_map_off, d_maps, d_sel, reinterpret_cast<uint64_t*>(d_pos), (hipStream_t)stream);
  });
}

int awry_dev_map_select_clip(awry_index_t* idx, int slot, const uint64_t* d_aln_off, const awry_aln_clip_t* d_alns, const awry_chain_t* d_chains,
                             const uint8_t* d_chain_status, uint64_t n, uint32_t chains_per_strand, uint32_t max_report, uint32_t match, uint32_t mismatch,
                             uint32_t gap, uint32_t end_bonus, uint32_t min_aln_score, uint64_t* d_n_maps, uint8_t* d_read_status, const uint64_t* d_map_off,
                             awry_map_clip_t* d_maps, uint32_t* d_sel, awry_pos_t* d_pos, void* stream) {
  return guarded([&] {
    require_map_args(chains_per_strand, max_report, 0);
    const MapMode mm = clip_map_mode(clip_mode(match, mismatch, gap, end_bonus), min_aln_score);
    Replica& r = replica(idx, slot);
    require(n == 0 || (d_aln_off && d_alns && d_chains && (d_map_off ? d_maps != nullptr : d_n_maps != nullptr)), "null device pointer");
    launch_map_select(r, d_aln_off, d_alns, reinterpret_cast<const Chain*>(d_chains), d_chain_status, n, chains_per_strand, max_report, mm, d_n_maps,
                      d_read_status, d_map_off, d_maps, d_sel, reinterpret_cast<uint64_t*>(d_pos), (hipStream_t)stream);
  });
}

int awry_dev_map_select_split(awry_index_t* idx, int slot, const uint64_t* d_aln_off, const awry_aln_clip_t* d_alns, const awry_chain_t* d_chains,
                              const uint8_t* d_chain_status, const uint64_t* d_qoff, uint64_t n, uint32_t chains_per_strand, uint32_t max_segments,
                              uint32_t max_secondary, uint32_t max_overlap, uint32_t match, uint32_t mismatch, uint32_t min_aln_score, uint64_t* d_n_maps,
                              uint8_t* d_read_status, const uint64_t* d_map_off, awry_map_split_t* d_maps, uint32_t* d_sel, awry_pos_t* d_pos, void* stream) {
  return guarded([&] {
    const SplitParams sp = split_params(chains_per_strand, max_segments, max_secondary, max_overlap, 0);
    const MapMode mm = clip_map_mode(clip_mode(match, mismatch, 0, 0), min_aln_score);
    Replica& r = replica(idx, slot);
    require(n == 0 || (d_aln_off && d_alns && d_chains && d_qoff && (d_map_off ? d_maps != nullptr : d_n_maps != nullptr)), "null device pointer");
    launch_map_split_select(r, d_aln_off, reinterpret_cast<const AlnClip*>(d_alns), reinterpret_cast<const Chain*>(d_chains), d_chain_status, d_qoff, 1, n,
                            chains_per_strand, sp, mm, d_n_maps, d_read_status, d_map_off, reinterpret_cast<MapSplitRec*>(d_maps), d_sel,
                            reinterpret_cast<uint64_t*>(d_pos), (hipStream_t)stream);
  });
}

int awry_dev_pair_windows(awry_index_t* idx, int slot, const uint64_t* d_cand_off, const awry_map_t* d_cands, const uint64_t* d_qoff, uint64_t n_pairs,
                          uint64_t min_insert, uint64_t max_insert, uint32_t rescue_anchors, int rescue_edits, uint32_t* d_win_query, uint64_t* d_win_first,
                          uint32_t* d_win_count, void* stream) {
  return guarded([&] {
    dev_pair_windows<MapRec>(idx, slot, d_cand_off, d_cands, d_qoff, n_pairs, min_insert, max_insert, rescue_anchors, rescue_edits, d_win_query, d_win_first,
                             d_win_count, stream);
  });
}

int awry_dev_pair_windows_clip(awry_index_t* idx, int slot, const uint64_t* d_cand_off, const awry_map_clip_t* d_cands, const uint64_t* d_qoff,
                               uint64_t n_pairs, uint64_t min_insert, uint64_t max_insert, uint32_t rescue_anchors, int rescue_edits, uint32_t* d_win_query,
                               uint64_t* d_win_first, uint32_t* d_win_count, void* stream) {
  return guarded([&] {
    dev_pair_windows<MapClipRec>(idx, slot, d_cand_off, d_cands, d_qoff, n_pairs, min_insert, max_insert, rescue_anchors, rescue_edits, d_win_query,
                                 d_win_first, d_win_count, stream);
  });
}

int awry_dev_pair_select(awry_index_t* idx, int slot, const uint64_t* d_cand_off, const awry_map_t* d_cands, const awry_map_t* d_resc,
                         const uint8_t* d_read_status, uint64_t n_pairs, uint64_t min_insert, uint64_t max_insert, uint32_t unpaired_penalty,
                         uint32_t rescue_anchors, uint64_t* d_n_maps, const uint64_t* d_map_off, awry_map_t* d_maps, uint32_t* d_sel, awry_pos_t* d_pos,
                         uint32_t* d_insert, void* stream) {
  return guarded([&] {
    const PairParams pp = pair_params(min_insert, max_insert, unpaired_penalty, rescue_anchors, 0);
    dev_pair_select<MapRec>(idx, slot, d_cand_off, d_cands, d_resc, d_read_status, n_pairs, pp, PairMode{}, d_n_maps, d_map_off, d_maps, d_sel, d_pos,
                            d_insert, stream);
  });
}

int awry_dev_pair_select_clip(awry_index_t* idx, int slot, const uint64_t* d_cand_off, const awry_map_clip_t* d_cands, const awry_map_clip_t* d_resc,
                              const uint8_t* d_read_status, uint64_t n_pairs, uint64_t min_insert, uint64_t max_insert, uint32_t unpaired_penalty,
                              uint32_t rescue_anchors, uint32_t match, uint32_t mismatch, uint32_t gap, uint32_t end_bonus, uint32_t min_aln_score,
                              uint64_t* d_n_maps, const uint64_t* d_map_off, awry_map_clip_t* d_maps, uint32_t* d_sel, awry_pos_t* d_pos, uint32_t* d_insert,
                              void* stream) {
  return guarded([&] {
    const PairParams pp = pair_params(min_insert, max_insert, unpaired_penalty, rescue_anchors, 0, true);
    const AlignMode md = clip_mode(match, mismatch, gap, end_bonus);
    dev_pair_select<MapClipRec>(idx, slot, d_cand_off, d_cands, d_resc, d_read_status, n_pairs, pp, clip_pair_mode(md, clip_map_mode(md, min_aln_score)),
                                d_n_maps, d_map_off, d_maps, d_sel, d_pos, d_insert, stream);
  });
}

int awry_debug_rank_all(awry_index_t* idx, int slot, const void* d_rows, uint64_t n, void* d_occ, void* stream) {
  return guarded([&] {
    Replica& r = replica(idx, slot);
    if (n == 0) return;
    require(d_rows && d_occ, "null argument");
    const dim3 g(grid_for(r, n, 256)), b(256);
    with_alphabet(r.dev.alphabet, [&](auto A) {
      hipLaunchKernelGGL(rank_all_kernel<A()>, g, b, 0, (hipStream_t)stream, r.dev, (const uint64_t*)d_rows, n, (uint64_t*)d_occ);
    });
    HIP_CHECK(hipGetLastError());
  });
}

int awry_dev_phase_marker(awry_index_t* idx, int slot, int phase_id, void* stream) {
  return guarded([&] {
    replica(idx, slot);
    require(phase_id >= 1 && phase_id <= 65535, "phase id out of range");
    hipLaunchKernelGGL(phase_marker_kernel, dim3((unsigned)phase_id), dim3(64), 0, (hipStream_t)stream);
    HIP_CHECK(hipGetLastError());
  });
}

int awry_dev_malloc(awry_index_t* idx, int slot, uint64_t bytes, void** d_out) {
  return guarded([&] { replica(idx, slot); require(d_out != nullptr, "null argument"); HIP_CHECK(hipMalloc(d_out, std::max<uint64_t>(bytes, 8))); });
}
int awry_dev_free(awry_index_t* idx, int slot, void* d) {
  return guarded([&] { replica(idx, slot); if (d) HIP_CHECK(hipFree(d)); });
}
int awry_dev_memcpy_h2d(awry_index_t* idx, int slot, void* d_dst, const void* h_src, uint64_t bytes) {
  return guarded([&] { replica(idx, slot); if (bytes) HIP_CHECK(hipMemcpy(d_dst, h_src, bytes, hipMemcpyHostToDevice)); });
}
int awry_dev_memcpy_d2h(awry_index_t* idx, int slot, void* h_dst, const void* d_src, uint64_t bytes) {
  return guarded([&] { replica(idx, slot); if (bytes) HIP_CHECK(hipMemcpy(h_dst, d_src, bytes, hipMemcpyDeviceToHost)); });
}
int awry_dev_memset(awry_index_t* idx, int slot, void* d_dst, int value, uint64_t bytes) {
  return guarded([&] { replica(idx, slot); if (bytes) HIP_CHECK(hipMemset(d_dst, value, bytes)); });
}
int awry_dev_synchronize(awry_index_t* idx, int slot) {
  return guarded([&] { replica(idx, slot); HIP_CHECK(hipDeviceSynchronize()); });
}
int awry_dev_stream_copy(awry_index_t* idx, int slot, void* d_dst, const void* d_src, uint64_t bytes, void* stream) {
  return guarded([&] {
    Replica& r = replica(idx, slot);
    require(d_dst && d_src && bytes % 16 == 0, "stream copy needs device pointers and a multiple of 16 bytes");
    hipLaunchKernelGGL(stream_copy_kernel, dim3((unsigned)r.num_cus * 16), dim3(256), 0, (hipStream_t)stream, (const uint4*)d_src, (uint4*)d_dst, bytes / 16);
    HIP_CHECK(hipGetLastError());
  });
}
int awry_dev_timer_begin(awry_index_t* idx, int slot, void* stream) {
  return guarded([&] { Replica& r = replica(idx, slot); HIP_CHECK(hipEventRecord(r.ev0, (hipStream_t)stream)); });
}
int awry_dev_timer_end(awry_index_t* idx, int slot, void* stream, float* ms_out) {
  return guarded([&] {
    Replica& r = replica(idx, slot);
    require(ms_out != nullptr, "null argument");
    HIP_CHECK(hipEventRecord(r.ev1, (hipStream_t)stream));
    HIP_CHECK(hipEventSynchronize(r.ev1));
    HIP_CHECK(hipEventElapsedTime(ms_out, r.ev0, r.ev1));
  });
}

}  // extern "C"
