// replica.h -- the pipeline lanes, the device replica of an index, awry_index and what every part asks of a replica
// A part of awry_hip.hip (one translation unit): included there, in order, and not on its own.
#pragma once

namespace {

// one pipeline lane of the host count paths (count_shard_hostpacked, count_shard_generic_pipelined): buffers persist in the
// replica and only grow
struct PackedLane {
  hipStream_t s = nullptr;  // owned by the replica
  hipEvent_t done = nullptr;
  hipEvent_t ev_in = nullptr, ev_k = nullptr;  // copy-in stream -> lane stream, lane stream -> copy-out stream (Replica::copy_in / copy_out)
  DevBuf<uint8_t> ascii;
  DevBuf<uint64_t> words, counts, off;  // off / lens: batches of unequal lengths
  DevBuf<uint32_t> lens, bad_list;      // bad_list: the chunk's queries with bytes outside ACGT
  DevBuf<uint8_t> status;               // generic kernel: per-query status of the chunk
  DevBuf<unsigned long long> bad;       // [1] first rejected query (index << 8 | status) or ~0
  unsigned long long* h_bad = nullptr;  // pinned copy
  // host-packed path (count_shard_hostpacked): persistent pinned staging, so that no caller memory is ever registered --
  // packed words in, counts out, and the compact copy (indices, offsets, bytes) of the chunk's queries with other letters
  PinBuf<uint64_t> h_words, h_boff;
  PinBuf<uint32_t> h_counts32, h_lens, h_bq;  // counts cross PCIe as 32-bit words and are widened into counts_out
  DevBuf<uint32_t> counts32;
  PinBuf<uint8_t> h_bbytes;
  DevBuf<uint8_t> bbytes;
  DevBuf<uint64_t> boff;
  uint64_t nbad = 0;
  uint64_t chunk_lo = 0, chunk_hi = 0;
  bool busy = false;
  ~PackedLane() {
    if (done) (void)hipEventDestroy(done);
    if (ev_in) (void)hipEventDestroy(ev_in);
    if (ev_k) (void)hipEventDestroy(ev_k);
    if (h_bad) (void)hipHostFree(h_bad);
  }
};

// one pipeline lane of the packed host locate path (locate_shard_packed); persists in the replica
struct LocateLane {
  hipEvent_t counted = nullptr, located = nullptr;
  hipEvent_t ev_in = nullptr, ev_k = nullptr;  // copy-in stream -> lane stream, lane stream -> copy-out stream (Replica::copy_in / copy_out)
  DevBuf<uint8_t> ascii;
  DevBuf<uint64_t> words, rstart, counts, hit_off, scratch, gpos, pos, off;
  DevBuf<uint32_t> lens, bad_list;
  DevBuf<uint8_t> status;                      // generic kernel: per-query status of the chunk,
  PinBuf<uint8_t> h_status;                    //   and where the host reads it
  DevBuf<unsigned long long> bad;              // [0] reads with bytes outside ACGT, [1] first rejected read (index << 8 | status) or ~0
  PinBuf<uint64_t> h_meta;                     // [0] total hits of the chunk, [1..2] copy of `bad`
  // host-packed reads: pinned staging of the packed words / lengths and the compact copy of the reads with other letters
  PinBuf<uint64_t> h_words, h_boff;
  PinBuf<uint32_t> h_lens, h_bq;
  PinBuf<uint8_t> h_bbytes;
  DevBuf<uint8_t> bbytes;
  DevBuf<uint64_t> boff;
  uint64_t lo = 0, hi = 0, total = 0;
  int stage = 0;                               // 0 idle, 1 count queued, 2 locate queued
  ~LocateLane() {
    if (counted) (void)hipEventDestroy(counted);
    if (located) (void)hipEventDestroy(located);
    if (ev_in) (void)hipEventDestroy(ev_in);
    if (ev_k) (void)hipEventDestroy(ev_k);
  }
};

struct Replica {
  int device = -1;
  hipStream_t stream = nullptr;
  static constexpr int NLANES = 3;
  hipStream_t lane_stream[NLANES] = {nullptr, nullptr, nullptr};  // the pipeline lanes of the host paths (locate uses two)
  // All chunk copies of the host-packed count path go through these two, one per direction, tied to the lanes' kernels by
  // events.  With the copies on the lane streams themselves, three streams copied at once, and after an accelerator rebuild
  // (or on a second replica) ONE of them was left on a copy path 2-3x slower (chunk in: 75-150 -> 250-300 us, out: 40-80 ->
  // 160-200 us; rocprofv3 --memory-copy-trace, profiles/r03a1_*), which then set the pace of every call: 1.45 -> 2.25 ms per
  // 5 M 31-mers, for good.  PCIe is the limit either way and one stream per direction sustains it.
  hipStream_t copy_in = nullptr, copy_out = nullptr;
  PackedLane lanes[NLANES];
  LocateLane loc_lanes[2];
  std::mutex lane_mu;  // one packed host call at a time per replica
  // single-query calls (count_string, search_range): a pinned mailbox the generic kernel reads and writes in place --
  // one launch and one stream synchronisation per call, no device allocation, no copies
  struct Mailbox {
    static constexpr size_t QCAP = 1 << 16;
    static constexpr size_t HCAP = 1 << 15;  // hits a single-query locate returns through the mailbox
    uint8_t* q = nullptr;       // [QCAP + 16]
    uint64_t* words = nullptr;  // off[2], count, range[2], status, hit_off[2]
    uint64_t* gpos = nullptr;   // [HCAP]
    uint64_t* pos = nullptr;    // [2 * HCAP]
    ~Mailbox() {
      for (void* p : {(void*)q, (void*)words, (void*)gpos, (void*)pos})
        if (p) (void)hipHostFree(p);
    }
  } mailbox;
  std::mutex mailbox_mu;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  DevBuf<uint64_t> blocks, sa_words, seq_starts;
  DevBuf<uint32_t> seq_bucket;  // DevIndex::seq_bucket (indexes of more records than the locate kernels keep in LDS)
  DevBuf<SeedEntry> seed;
  DevBuf<SeedEntry64> seed64;  // wide-row replicas (bwt_len >= 2^32, or forced): 16-byte entries
  // seed tables for k-mers SHORTER than the main table's k ("rungs": one complete 4^L table per query length L that has
  // been asked for, built on first use; a 12-mer is then answered by its entry instead of 12 LF steps)
  std::map<int, DevBuf<SeedEntry>> rungs;
  std::set<int> rungs_refused;  // lengths whose table did not fit the HBM budget when first asked for
  std::mutex rung_mu;
  // The k-mer count table (layout.h, KT_*): ONE per replica, for the query length it was last built for (accelerators.h,
  // kmer_table).  A launcher reads it under a shared lock that it holds until its kernel is queued; building, replacing and
  // dropping take the lock exclusively, and freeing the old table waits for the device -- so no kernel runs on a freed table.
  struct KmerTable {
    DevBuf<uint64_t> tab;
    int L = 0;
    uint32_t bits = 0;  // 2^bits lines of 16 entries
    uint64_t entries = 0, overflowed = 0;
    double build_ms = 0;
  } kt;
  std::set<int> kt_refused;  // lengths whose table did not fit the HBM budget when first asked for (forgotten with the table)
  std::shared_mutex kt_mu;
  int kt_mode = -1;          // awry_set_kmer_table: -1 policy, 0 off, 1 build for the next length whatever the batch size
  bool wide = false;          // 64-bit rows: wide kernels, no 32-bit accelerators
  DevBuf<uint32_t> text4;                     // 4-bit text for seed-and-verify (device-only accelerator)
  DevBuf<uint8_t> text8;                      // the text as symbol indices, for the generic kernel's verify (any alphabet)
  DevBuf<uint32_t> dense_sa;                  // SA[j * dense_ratio] as u32 (device-only accelerator for locate)
  DevBuf<uint32_t> sa_nblock;                 // SA of the rows whose suffix starts with N (kept while locate has to walk)
  DevBuf<uint64_t> lcx_key, lcx_rowpos, lcx_inner;  // left-context index (layout.h, DevIndex::lcx_key); kept with position seeds
  DevBuf<uint8_t> edit_text8;                 // the edit scan's own copy of the text while text8 is not resident (built on first use, edit_host.h)
  std::mutex edit_mu;
  uint32_t dense_ratio = 0;                   // 0 = use the file's bit-packed samples
  uint32_t verify_after = 0;                  // seed-and-verify: LF steps before the text comparison (DevIndex::verify_after)
  bool verify_kmers = false;                  // also use seed-and-verify in the k-mer (L <= 32) kernel
  // survivor lists of the two-phase count schedule, one per stream (launches on one stream are ordered, so reuse is safe)
  struct SurvScratch {
    DevBuf<uint64_t> w, range;
    DevBuf<uint32_t> q, count;
    uint64_t cap = 0, cap_q = 0;
    // what lcx_quad_reads_kernel leaves for the LF pass: one device-wide list (fcount[0] slots used, fcap allocated:
    // lcx_lf_list_bound of the launch)
    DevBuf<uint64_t> fw, frange;
    DevBuf<uint32_t> fq, fcount;
    uint64_t fcap = 0;
    // awry_dev_count_ascii_uniform on a nucleotide index: packed words of the batch, the pack kernel's list of queries with
    // other letters and its counter
    DevBuf<uint64_t> u_words;
    DevBuf<uint32_t> u_list;
    DevBuf<unsigned long long> u_bad;
    // count_dfs_kernel<CLASSES>: the DFS frames below the two a lane keeps in registers, [level][field][grid lane]
    DevBuf<uint64_t> pat_stack;
    // edit_scan_kernel: the pattern masks edit_masks_kernel writes in front of it, per query or per window
    DevBuf<uint64_t> edit_masks;
    // edit_align_kernel: one direction word per table row and grid lane, [row][grid lane] (sized by the grid, launchers.h)
    DevBuf<uint64_t> align_trace;
    // chain_kernel: the working sets of queries beyond the LDS tile, one slab per group of the grid (sized by the grid, launchers.h)
    DevBuf<uint8_t> chain_slabs;
    // chain_align_kernel: the class lists chain_align_classify_kernel writes in front of it -- [class][chain index], then the
    // three list lengths (launchers.h); its direction words go to align_trace
    DevBuf<uint32_t> chain_align_lists;
    // work-queue heads of the chunk / locate kernels launched on this stream: launches on one stream are ordered, so a
    // head is free again by the time the ring comes back to it, however many launches other streams have in flight
    DevBuf<unsigned long long> counters;
    unsigned counter_seq = 0;
    // Held by a launch helper from the moment it reads these buffers until its kernels are queued (ScratchLock), growth
    // included: two host threads that drive ONE stream -- the replica's own in the unpipelined host drivers, the NULL stream
    // of two device-resident callers -- then never launch with a list the other has just freed.  Recursive: the uniform entry
    // point holds it around the packed launchers, which take it again.  Never contended when a stream has one driver.
    std::recursive_mutex mu;
  };
  std::mutex scratch_mu;  // the map below and the head ring's sequence numbers
  std::map<hipStream_t, std::unique_ptr<SurvScratch>> scratch;
  int seed_k = 0;
  bool seed_pos = false;        // the seed table's singletons hold text positions (DevIndex::seed_pos) ...
  int ctx_extra = 0;            // ... with this many context letters beyond 14 (DevIndex::ctx_extra)
  uint32_t lcx_off[8] = {0};    // the levels of lcx_inner (DevIndex::lcx_off)
  int num_cus = 256;
  // blocks of count_nt2_probe_resume_kernel<TALLY, VERIFY> resident per CU, by [2 * TALLY + VERIFY] (the occupancy query of
  // each instantiation, at replica creation): its grid, and the number of survivor lists two_phase_lists sizes
  int probe_resume_per_cu[4] = {8, 8, 8, 8};
  // blocks of lcx_quad_reads_kernel<RAGGED> resident at once, by [RAGGED] (the occupancy query at replica creation): its
  // grid, and the number of waves whose partly filled chunks two_phase_lists makes room for in the LF list
  unsigned lcx_reads_grid[2] = {0, 0};
  // The kernels' view.  The index fields are written once (accelerators.h upload_index); every accelerator field is written by
  // publish() alone, from the buffers and the host-side state above.
  DevIndex dev{};
  ~Replica() {
    if (device >= 0) {
      (void)hipSetDevice(device);
      if (stream) (void)hipStreamDestroy(stream);
      for (auto& ls : lane_stream) if (ls) (void)hipStreamDestroy(ls);
      if (copy_in) (void)hipStreamDestroy(copy_in);
      if (copy_out) (void)hipStreamDestroy(copy_out);
      if (ev0) (void)hipEventDestroy(ev0);
      if (ev1) (void)hipEventDestroy(ev1);
      blocks.reset(); sa_words.reset(); seq_starts.reset(); seed.reset(); seed64.reset(); rungs.clear(); dense_sa.reset(); text4.reset();
      scratch.clear();
      sa_nblock.reset(); text8.reset(); edit_text8.reset();
      lcx_key.reset(); lcx_rowpos.reset(); lcx_inner.reset();
      kt.tab.reset();
    }
  }
};

}  // namespace

struct awry_index {
  HostIndex host;
  std::vector<std::unique_ptr<Replica>> reps;
  int seed_k_request = -1;      // -1 = default policy
  int dense_ratio_request = 0;  // 0 = locate walks to the file's SA samples
  int verify_request = -2;      // -2: policy; -1: seed-and-verify off; >= 0: LF steps before switching to text comparison
  bool verify_kmers_request = false;
  int lcx_request = -1;         // -1: policy (on when it fits); 0: no left-context index; 1: as -1
  int kmer_table_request = -1;  // awry_set_kmer_table (Replica::kt_mode)
};

namespace {

Replica& replica(awry_index* ix, int slot) {
  require(ix != nullptr, "null index");
  if (ix->reps.empty()) throw NoDeviceError("no device replica: call awry_set_devices() first (there is no CPU search path)");
  require(slot >= 0 && slot < (int)ix->reps.size(), "replica slot out of range");
  Replica& r = *ix->reps[slot];
  HIP_CHECK(hipSetDevice(r.device));
  return r;
}

// awry_debug_set_max_blocks: an upper bound on the block count of a launch, read at every launch; 0 (the default): none.  For
// tests: on a grid of one block every lane of a stride loop takes item after item, and scratch indexed by grid lane is reused
// from trip to trip, at batches of a few hundred items.  It bounds grid_for, resident_grid and the block counts the launchers
// of launchers.h work out themselves from num_cus or a byte budget (launch_locate, launch_chain, launch_chain_align,
// launch_edit_align); scratch sized from such a grid is sized from the bounded one.  It does not bound grids that are a function
// of the data (launch_scan: one tile per block) nor the grids of the k-mer count schedules (num_cus * 8 lists, probe_resume_per_cu,
// lcx_reads_grid), whose list layout is tied to the block count, nor the other grids a call site writes out itself from num_cus
// (the amino two-phase schedule, the LIST_GLOBAL pass of count_scalar_kernel, stream_copy_kernel).
std::atomic<int> g_max_blocks{0};
uint64_t bound_blocks(uint64_t blocks) {
  const int m = g_max_blocks.load();
  return m > 0 ? std::min<uint64_t>(blocks, (uint64_t)m) : blocks;
}

int grid_for(const Replica& r, uint64_t work_items, int per_block, int blocks_per_cu = 8) {
  uint64_t want = (work_items + per_block - 1) / per_block;
  uint64_t cap = bound_blocks((uint64_t)r.num_cus * blocks_per_cu);
  return (int)std::max<uint64_t>(1, std::min(want, cap));
}

// Rows fit 32 bits: the packed kernels, seed entries and accelerators are the 32-bit ones.  awry_debug_force_wide_rows(1)
// makes replicas built afterwards take the wide-row (64-bit) kernels whatever their size -- how those kernels are tested,
// since an index of 2^32 rows takes an hour of host SA-IS to build (the GPU builder stops below 2^32).
std::atomic<int> g_force_wide{0};
bool narrow(const HostIndex& h) { return h.bwt_len < (1ull << 32) - 512 && !g_force_wide.load(); }

// HBM the accelerator policies may plan with on the current device (accel_plan.h HbmFree): what is free now, capped by
// AWRY_HBM_BUDGET_GB (a process that shares the GPU, or wants room for its own buffers, sets it; the seed table is sized to
// 70 % and the verify accelerators admitted below 50 % of this figure)
HbmFree hbm_free() {
  size_t free_b = 0, total_b = 0;
  if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return HbmFree{};
  if (const char* e = getenv("AWRY_HBM_BUDGET_GB")) {
    const double gb = atof(e);
    if (gb > 0) free_b = std::min<size_t>(free_b, (size_t)(gb * 1e9));
  }
  return HbmFree{true, free_b};
}

// survivor lists of the two-phase schedules, one set per stream
Replica::SurvScratch* surv_scratch(Replica& r, hipStream_t s) {
  std::lock_guard<std::mutex> lock(r.scratch_mu);
  auto& slot = r.scratch[s];
  if (!slot) slot = std::make_unique<Replica::SurvScratch>();
  return slot.get();
}

// exclusive use of the scratch of stream `s` for the rest of the scope: read, grow and launch as one step (SurvScratch::mu)
struct ScratchLock {
  std::unique_lock<std::recursive_mutex> lk;
  ScratchLock(Replica& r, hipStream_t s) : lk(surv_scratch(r, s)->mu) {}
};

// The next head of the stream's ring of 8, zeroed by a memset queued on the stream.  The caller holds the stream's ScratchLock
// from here until the kernel that draws from the head is queued: otherwise a second host thread on the stream could take 8 heads
// in between, and two kernels would be queued behind both memsets of one head -- the second starts from the count the first left.
unsigned long long* next_counter(Replica& r, hipStream_t s) {
  Replica::SurvScratch* sc = surv_scratch(r, s);
  unsigned long long* ctr;
  {
    std::lock_guard<std::mutex> lock(r.scratch_mu);
    if (!sc->counters.p) sc->counters.alloc(8);
    ctr = sc->counters.p + (sc->counter_seq++ & 7u);
  }
  HIP_CHECK(hipMemsetAsync(ctr, 0, 8, s));
  return ctr;
}

}  // namespace
