// launchers.h -- every kernel launch helper (all asynchronous on the stream they are given); the packed count launchers run
// the schedule count_plan.h chooses
// A part of awry_hip.hip (one translation unit): included there, in order, and not on its own.
#pragma once

namespace {

// the schedule forced on the packed count launchers (CountFacts::forced in count_plan.h has the numbers)
std::atomic<int> g_count_kernel{-1};
// -1: no explicit choice (env / policy)
int count_kernel_override() {
  int m = g_count_kernel.load();
  if (m >= 0) return m;
  const char* e = getenv("AWRY_COUNT_KERNEL");
  if (e && !strcmp(e, "strided")) return 0;
  if (e && !strcmp(e, "chunk")) return 1;
  if (e && !strcmp(e, "quad4")) return 2;
  if (e && !strcmp(e, "twophase")) return 3;
  return -1;
}

// what plan_kmers / plan_reads (count_plan.h) read of a replica
CountFacts count_facts(const Replica& r) {
  static const bool rungs_off = getenv("AWRY_SEED_RUNGS") && !strcmp(getenv("AWRY_SEED_RUNGS"), "0");
  static const bool table_off = getenv("AWRY_KMER_TABLE") && !strcmp(getenv("AWRY_KMER_TABLE"), "0");
  CountFacts f;
  f.alphabet = r.dev.alphabet;
  f.wide = r.wide;
  f.bwt_len = r.dev.bwt_len;
  f.seed_k = r.seed_k;
  f.seed = r.seed.p != nullptr;
  f.seed64 = r.dev.seed64 != nullptr;
  f.text4 = r.dev.text4 != nullptr;
  f.dense_ratio = r.dev.dense_ratio;
  f.lcx_key = r.dev.lcx_key != nullptr;
  f.kt_mode = r.kt_mode;
  f.verify_kmers = r.verify_kmers;
  f.num_cus = r.num_cus;
  for (int i = 0; i < 4; i++) f.probe_resume_per_cu[i] = r.probe_resume_per_cu[i];
  for (int i = 0; i < 2; i++) f.lcx_reads_grid[i] = r.lcx_reads_grid[i];
  f.forced = count_kernel_override();
  f.rungs_off = rungs_off;
  f.table_off = table_off;
  return f;
}
// the grid of a plan's launches (the lane pass has p.lcx_grid): its block count, or sized from the batch
dim3 plan_grid(const Replica& r, const CountPlan& p, uint64_t n) {
  return dim3(p.blocks ? p.blocks : (unsigned)grid_for(r, n * p.items_per_query, 256));
}

// ---- kernel launch helpers (all asynchronous on `s`) ------------------------------------------------

// ASCII -> packed 2-bit words.  d_off == nullptr: n queries of L bytes each; else query q = bytes [d_off[q] - base, d_off[q+1] - base)
// of d_ascii (total_bytes in all), W words per query (stride), lengths to d_lens.
void launch_pack_nt2(Replica& r, const uint8_t* d_ascii, const uint64_t* d_off, uint64_t base, uint64_t n, uint64_t total_bytes, int L, int W,
                     uint64_t* d_words, uint32_t* d_lens, unsigned long long* d_bad, hipStream_t s, uint32_t* d_bad_list = nullptr) {
  if (n == 0) return;
  const dim3 g(grid_for(r, (n + 63) / 64 * 64, 256)), b(256);
  with_flags(d_off != nullptr, [&](auto R) {
    hipLaunchKernelGGL(pack_nt2_tile_kernel<R()>, g, b, 0, s, d_ascii, d_off, base, n, total_bytes, L, W, d_words, d_lens, d_bad, d_bad_list);
  });
  HIP_CHECK(hipGetLastError());
}

// The amino k-mer schedule: count_aa_kmer_probe_kernel (one query per lane: the seed entry, or the entry plus a text
// window, decides most) and the generic kernel over what it listed, as one pool.  d_off == nullptr: n queries of L residues
// back to back; else query q = d_q[d_off[q], d_off[q + 1]) of any length (k .. 24 residues take the first pass, the rest
// is listed).  d_ranges (optional): RS_* words / row starts for the locate pass, in the generic kernel's layout.
void launch_aa_two_phase(Replica& r, const uint8_t* d_q, const uint64_t* d_off, uint64_t n, int L, uint64_t* d_counts, uint64_t* d_ranges,
                         uint8_t* d_status, hipStream_t s, unsigned long long* d_tally) {
  const ScratchLock scratch_lock(r, s);
  Replica::SurvScratch* sc = surv_scratch(r, s);
  const unsigned nblk = (unsigned)r.num_cus * 8;
  const uint64_t per_block = list_slots_per_block(n, nblk);
  if (sc->cap_q < per_block * nblk) {
    HIP_CHECK(hipStreamSynchronize(s));
    sc->q.alloc(per_block * nblk);
    sc->cap_q = per_block * nblk;
    sc->cap = 0;  // the nucleotide k-mer path re-allocates its three lists together
  }
  if (!sc->count.p) sc->count.alloc(nblk);
  // the second pass works through all lists as one pool on a grid sized to what is resident at once (3 blocks per CU)
  const bool pooled = nblk <= (unsigned)LIST_MAX_LISTS;
  const QueryList ql{sc->q.p, sc->count.p, per_block, nullptr, nullptr, 0, d_tally, pooled ? nblk : 0u};
  const unsigned nblk2 = pooled ? (unsigned)r.num_cus * 3 : nblk;
  // Two queries in flight per lane (one: the same rate; four: 141 VGPRs, 10 % slower).  The second pass is a latency
  // chain over a few per cent of the batch; running it for the first half of a batch on a side stream beside the first
  // pass of the second half (event fork / join) was measured and costs more than it hides (12.7 -> 10.7 G present
  // 12-mers/s, host path 0.83 -> 0.52 G queries/s).
  // queries of more than 24 residues (up to AA_KMER_LONG_MAX): the LONG instantiations -- the same pass over a query's last 24
  // residues plus a comparison of the rest with the text for the candidates that are left
  static const bool no_long = getenv("AWRY_AA_LONG") && !strcmp(getenv("AWRY_AA_LONG"), "0");
  const bool lng = d_off ? !no_long : L > AA_KMER_MAX;
  with_flags(d_off != nullptr, lng, [&](auto R, auto G) {
    hipLaunchKernelGGL((count_aa_kmer_probe_kernel<2, R(), G()>), dim3(nblk), dim3(256), 0, s, r.dev, d_q, d_off, n, d_off ? 0 : L, d_counts, d_ranges, d_status, ql);
  });
  hipLaunchKernelGGL((count_scalar_kernel<AMINO, LIST_BLOCK>), dim3(nblk2), dim3(256), 0, s, r.dev, d_q, d_off, n, d_counts, d_ranges, d_status, 1,
                     d_off ? 0 : (uint64_t)L, ql);
  HIP_CHECK(hipGetLastError());
}

// allow_verify: the generic kernel may finish queries against the text (ranges then hold RS_* words for locate, not rows)
// ulen != 0: n queries of ulen bytes each, back to back (d_off is not read)
// ref_kmer_len >= 0: the reference's own step schedule with that lookup_table_kmer_len -- no seed table, kmer_len - 1 steps taken
// unconditionally (src/fm_index.rs:402-438, src/kmer_lookup_table.rs:90-110): what awry_search_range returns, rows of absent queries included
void launch_count_ascii(Replica& r, const uint8_t* d_q, const uint64_t* d_off, uint64_t n, uint64_t* d_counts,
                        uint64_t* d_ranges, uint8_t* d_status, hipStream_t s, bool allow_verify, uint64_t ulen = 0, int ref_kmer_len = -1) {
  if (n == 0) return;
  const int vmode = ref_kmer_len >= 0 ? (2 | (ref_kmer_len << 8)) : (allow_verify ? 1 : 0);
  if (ref_kmer_len >= 0) allow_verify = false;
  static const bool aa_off = getenv("AWRY_AA_KMER") && !strcmp(getenv("AWRY_AA_KMER"), "0");
  if (r.dev.alphabet == AMINO && allow_verify && !ulen && d_off && r.seed_k >= 1 && n >= 4096 && n < (1ull << 32) && !aa_off) {
    // amino batches of any lengths: the k-mer schedule with per-query lengths (queries it does not take are listed)
    launch_aa_two_phase(r, d_q, d_off, n, 0, d_counts, d_ranges, d_status, s, nullptr);
    return;
  }
  const dim3 g(grid_for(r, n, 256)), b(256);
  const QueryList none{};
  with_alphabet(r.dev.alphabet, [&](auto A) {
    hipLaunchKernelGGL((count_scalar_kernel<A(), LIST_NONE>), g, b, 0, s, r.dev, d_q, d_off, n, d_counts, d_ranges, d_status, vmode, ulen, none);
  });
  HIP_CHECK(hipGetLastError());
}

uint64_t scan_tiles(uint64_t n) { return (n + SCAN_TILE - 1) / SCAN_TILE; }

void launch_scan(Replica& r, const uint64_t* d_counts, uint64_t n, uint64_t* d_hit_off, uint64_t* d_scratch, hipStream_t s) {
  if (n == 0) { HIP_CHECK(hipMemsetAsync(d_hit_off, 0, 8, s)); return; }
  const uint64_t tiles = scan_tiles(n);
  hipLaunchKernelGGL(scan_tile_sums_kernel, dim3((unsigned)tiles), dim3(256), 0, s, d_counts, n, d_scratch);
  hipLaunchKernelGGL(scan_tile_offsets_kernel, dim3(1), dim3(256), 0, s, d_scratch, tiles, d_scratch + tiles);
  hipLaunchKernelGGL(scan_apply_kernel, dim3((unsigned)tiles), dim3(256), 0, s, d_counts, n, d_scratch, d_hit_off);
  HIP_CHECK(hipGetLastError());
}

// d_range_start[q * rs_stride] = first BWT row of query q's range
void launch_locate(Replica& r, const uint64_t* d_range_start, int rs_stride, const uint64_t* d_hit_off, uint64_t n, uint64_t total,
                   uint64_t* d_gpos, uint64_t* d_pos, hipStream_t s, unsigned long long* d_tally = nullptr) {
  if (total == 0) return;
  // from the first head to the last kernel queued: a head's memset and the kernel that draws from it stay next to each other
  // on the stream when two host threads drive it (next_counter, replica.h)
  const ScratchLock scratch_lock(r, s);
  unsigned long long* ctr = next_counter(r, s);
  const uint64_t tiles = (total + LOC_TILE - 1) / LOC_TILE;
  const dim3 g((unsigned)std::min<uint64_t>(tiles, bound_blocks((uint64_t)r.num_cus * 8))), b(256);
  // consecutive tiles a block draws at a time (one search of the whole offset array per run): long enough to amortise
  // that search, short enough that every block still draws several runs and the launch ends evenly
  const uint32_t run_len = (uint32_t)std::min<uint64_t>(16, std::max<uint64_t>(1, tiles / ((uint64_t)g.x * 4)));
  const uint32_t* dense = r.dense_ratio ? r.dense_sa.p : nullptr;
  with_alphabet(r.dev.alphabet, [&](auto A) {
    hipLaunchKernelGGL(locate_tile_kernel<A()>, g, b, 0, s, r.dev, d_range_start, rs_stride, d_hit_off, n, total, dense, r.dense_ratio, d_gpos, d_pos, ctr, run_len);
  });
  HIP_CHECK(hipGetLastError());
  if (r.dense_ratio == 1) return;  // every row is a sampled row: nothing was deferred
  // the hits whose row is not sampled walk in a second pass that is not tied to tiles (locate_walk_kernel)
  unsigned long long* wctr = next_counter(r, s);
  if (r.dev.alphabet == NUCLEOTIDE)
    with_flags(d_tally != nullptr, [&](auto T) {
      hipLaunchKernelGGL((locate_walk_nt_lane_kernel<true, T()>), dim3(grid_for(r, total, 256, 4)), b, 0, s, r.dev, total, dense, r.dense_ratio, d_gpos, wctr, d_tally);
    });
  else hipLaunchKernelGGL(locate_walk_kernel<AMINO>, dim3(grid_for(r, total, 256, 7)), b, 0, s, r.dev, total, dense, r.dense_ratio, d_gpos, d_pos, wctr);
  if (d_pos) hipLaunchKernelGGL(localise_walked_kernel, dim3(grid_for(r, total, 256)), b, 0, s, r.dev, total, d_gpos, d_pos);
  HIP_CHECK(hipGetLastError());
}

// the survivor lists of a two-phase launch over n queries on a grid of nblk <= num_cus * 8 blocks (one list per block):
// `in` (all three arrays) and, with lcx_grid != 0, the LF list `out` of lcx_quad_reads_kernel on a grid of lcx_grid blocks.
// The caller holds the stream's ScratchLock until it has queued the kernels that take these pointers.
void two_phase_lists(Replica& r, hipStream_t s, uint64_t n, unsigned nblk, unsigned lcx_grid, Nt2Survivors* in, Nt2Survivors* out) {
  Replica::SurvScratch* sc = surv_scratch(r, s);
  const uint64_t per_block = list_slots_per_block(n, nblk), total = per_block * nblk;
  const uint64_t fneed = lcx_grid ? lcx_lf_list_bound(total, lcx_grid) : 0;
  if (sc->cap < total || sc->fcap < fneed) {
    HIP_CHECK(hipStreamSynchronize(s));
    if (sc->cap < total) {
      sc->w.alloc(total); sc->range.alloc(total); sc->q.alloc(total);
      sc->cap = sc->cap_q = total;
    }
    if (sc->fcap < fneed) {
      sc->fw.alloc(fneed); sc->frange.alloc(fneed); sc->fq.alloc(fneed);
      sc->fcap = fneed;
    }
  }
  if (!sc->count.p) sc->count.alloc((size_t)r.num_cus * 8);
  if (lcx_grid && !sc->fcount.p) sc->fcount.alloc(8);  // [0] length of the LF list
  *in = Nt2Survivors{sc->w.p, sc->range.p, sc->q.p, sc->count.p, per_block};
  *out = Nt2Survivors{};
  if (lcx_grid) {
    *out = Nt2Survivors{sc->fw.p, sc->frange.p, sc->fq.p, sc->fcount.p, sc->fcap};
    in->lf_count = sc->fcount.p;
  }
}
// blocks of a kernel that are resident at once: its grid (the work is shared out dynamically)
template <class K>
unsigned resident_grid(const Replica& r, K kernel) {
  int per_cu = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, 256, 0) != hipSuccess || per_cu < 1) { (void)hipGetLastError(); per_cu = 2; }
  return (unsigned)bound_blocks((uint64_t)r.num_cus * (unsigned)per_cu);
}

// Packed queries on a wide-row replica (64-bit rows), for both packed launchers: k-mers (one word, d_tally optional) and reads
// (d_lens, d_range_start optional).  The census is the k-mer path's: d_tally goes with equal lengths only.  The caller holds
// the stream's ScratchLock and has planned a wide schedule.
void launch_count_nt2_wide(Replica& r, const CountPlan& p, const uint64_t* d_words, uint64_t n, int L, uint64_t* d_counts, uint64_t* d_range_start,
                           hipStream_t s, const uint32_t* d_lens, unsigned long long* d_tally) {
  require(!(d_lens && d_tally), "internal: no census for reads of unequal lengths");
  const dim3 gw(plan_grid(r, p, n)), bw(256);
  if (p.schedule == CountSchedule::WIDE_TWO_PHASE) {
    Nt2Survivors sv, fb;
    two_phase_lists(r, s, n, p.blocks, 0u, &sv, &fb);
    if (d_lens) hipLaunchKernelGGL((count_nt2_wide_probe_kernel<true, false>), gw, bw, 0, s, r.dev, d_words, n, L, d_counts, d_range_start, sv, d_lens, d_tally);
    else with_flags(d_tally != nullptr, [&](auto T) {
      hipLaunchKernelGGL((count_nt2_wide_probe_kernel<false, T()>), gw, bw, 0, s, r.dev, d_words, n, L, d_counts, d_range_start, sv, d_lens, d_tally);
    });
    with_flags(d_lens != nullptr, [&](auto R) {
      hipLaunchKernelGGL((count_nt2_wide_kernel<true, R(), true>), gw, bw, 0, s, r.dev, d_words, n, L, d_counts, d_range_start, d_lens, d_tally, sv);
    });
  } else {
    require(p.schedule == CountSchedule::WIDE_SINGLE, "internal: not a wide-row schedule");
    with_flags(p.seeded, d_lens != nullptr, [&](auto S, auto R) {
      hipLaunchKernelGGL((count_nt2_wide_kernel<S(), R()>), gw, bw, 0, s, r.dev, d_words, n, L, d_counts, d_range_start, d_lens, d_tally);
    });
  }
  HIP_CHECK(hipGetLastError());
}

// d_lens != nullptr: read q has d_lens[q] letters (1..L) in its W = ceil(L / 32) words; else every read has L letters
void launch_count_nt2_long(Replica& r, const uint64_t* d_words, uint64_t n, int L, uint64_t* d_counts, uint64_t* d_range_start,
                           bool use_seed, hipStream_t s, const uint32_t* d_lens = nullptr) {
  require(r.dev.alphabet == NUCLEOTIDE, "packed 2-bit queries need a nucleotide index");
  require(L >= 1 && L <= 1 << 20, "packed read length out of range");
  if (n == 0) return;
  const ScratchLock scratch_lock(r, s);
  const CountPlan p = plan_reads(count_facts(r), n, L, use_seed, d_lens != nullptr);
  const dim3 g(plan_grid(r, p, n)), b(256);
  switch (p.schedule) {
    case CountSchedule::WIDE_SINGLE:
    case CountSchedule::WIDE_TWO_PHASE:
      launch_count_nt2_wide(r, p, d_words, n, L, d_counts, d_range_start, s, d_lens, nullptr);
      return;
    case CountSchedule::READS_LISTS:
    case CountSchedule::READS_LANES: {
      const bool lanes = p.schedule == CountSchedule::READS_LANES;
      Nt2Survivors sv, fb;
      two_phase_lists(r, s, n, p.blocks, p.lcx_grid, &sv, &fb);
      if (!lanes) sv.w = sv.range = nullptr;  // (the probe pass then lists the reads only)
      with_flags(d_lens != nullptr, [&](auto R) {
        hipLaunchKernelGGL(count_nt2_reads_probe_kernel<R()>, g, b, 0, s, r.dev, d_words, n, L, d_counts, d_range_start, sv, d_lens);
        if (lanes) {
          hipLaunchKernelGGL(lcx_quad_reads_kernel<R()>, dim3(p.lcx_grid), b, 0, s, r.dev, d_words, L, d_counts, d_range_start, sv, fb, p.blocks, d_lens);
          hipLaunchKernelGGL(count_nt2_reads_pool_kernel<R()>, g, b, 0, s, r.dev, d_words, L, d_counts, d_range_start, fb, d_lens);  // the quad code over what the lanes left
        } else hipLaunchKernelGGL((count_nt2_reads_kernel<true, true, true, R()>), g, b, 0, s, r.dev, d_words, n, L, d_counts, d_range_start, sv, d_lens);
      });
      break;
    }
    case CountSchedule::READS_SINGLE: {
      const Nt2Survivors none{};
      with_flags(p.seeded, p.verify, d_lens != nullptr, [&](auto S, auto V, auto R) {
        hipLaunchKernelGGL((count_nt2_reads_kernel<S(), V(), false, R()>), g, b, 0, s, r.dev, d_words, n, L, d_counts, d_range_start, none, d_lens);
      });
      break;
    }
    default: require(false, "internal: not a schedule for reads");
  }
  HIP_CHECK(hipGetLastError());
}

void launch_count_nt2(Replica& r, const uint64_t* d_words, uint64_t n, int L, uint64_t* d_counts, bool use_seed, hipStream_t s,
                      unsigned long long* d_tally = nullptr) {
  require(r.dev.alphabet == NUCLEOTIDE, "packed 2-bit queries need a nucleotide index");
  require(L >= 1 && L <= 32, "packed k-mer length must be in 1..32");
  if (n == 0) return;
  const ScratchLock scratch_lock(r, s);
  CountFacts f = count_facts(r);
  CountPlan p = plan_kmers(f, n, L, use_seed, d_tally != nullptr);
  // a wanted rung or count table of this length: resident, or built now (the table in place of another length's); where
  // that fails the launch is planned again without it.  The launch gets either in its own copy of the index.
  DevIndex dv = r.dev;
  std::shared_lock<std::shared_mutex> kt_lock;  // held until the kernel that takes the table is queued
  if (p.rung) {
    if (const SeedEntry* t = seed_rung(r, L)) { dv.seed = t; dv.seed_k = L; dv.seed_pos = 0; dv.ctx_extra = 0; }
    else { f.rung_failed = true; p = plan_kmers(f, n, L, use_seed, d_tally != nullptr); }
  }
  if (p.table) {
    if (const Replica::KmerTable* kt = kmer_table(r, L, true, kt_lock)) { dv.kmer_tab = kt->tab.p; dv.kmer_tab_bits = kt->bits; }
    else { f.table_failed = true; p = plan_kmers(f, n, L, use_seed, d_tally != nullptr); }
  }
  const dim3 g(plan_grid(r, p, n)), b(256);
  switch (p.schedule) {
    case CountSchedule::WIDE_SINGLE:
    case CountSchedule::WIDE_TWO_PHASE:
      launch_count_nt2_wide(r, p, d_words, n, L, d_counts, nullptr, s, nullptr, d_tally);
      return;
    case CountSchedule::LDS_CHUNKS: {
      unsigned long long* ctr = next_counter(r, s);
      with_flags(p.seeded, d_tally != nullptr, [&](auto S, auto T) {
        hipLaunchKernelGGL((count_nt2_chunk_kernel<S(), T()>), g, b, 0, s, r.dev, d_words, n, L, d_counts, ctr, d_tally);
      });
      break;
    }
    case CountSchedule::PROBE_RESUME:
    case CountSchedule::PROBE_THEN_RESUME: {  // (the one launch takes the survivor count from LDS and leaves sv.count untouched)
      Nt2Survivors sv, fb;
      two_phase_lists(r, s, n, p.blocks, 0u, &sv, &fb);
      with_flags(d_tally != nullptr, p.verify, [&](auto T, auto V) {
        if (p.schedule == CountSchedule::PROBE_THEN_RESUME) {
          hipLaunchKernelGGL((count_nt2_probe_kernel<T(), V()>), g, b, 0, s, dv, d_words, n, L, d_counts, sv, d_tally);
          hipLaunchKernelGGL((count_nt2_resume_kernel<T(), V()>), g, b, 0, s, dv, sv, L, d_counts, d_tally);
        } else hipLaunchKernelGGL((count_nt2_probe_resume_kernel<T(), V()>), g, b, 0, s, dv, d_words, n, L, d_counts, sv, d_tally);
      });
      break;
    }
    case CountSchedule::QUAD4:
      with_flags(p.seeded, d_tally != nullptr, p.verify, [&](auto S, auto T, auto V) {
        hipLaunchKernelGGL((count_nt2_quad4_kernel<S(), T(), V()>), g, b, 0, s, r.dev, d_words, n, L, d_counts, d_tally);
      });
      break;
    case CountSchedule::STRIDED_QUADS:
      with_flags(p.seeded, d_tally != nullptr, [&](auto S, auto T) {
        hipLaunchKernelGGL((count_nt2_quad_kernel<S(), T()>), g, b, 0, s, r.dev, d_words, n, L, d_counts, d_tally);
      });
      break;
    default: require(false, "internal: not a schedule for k-mers");
  }
  HIP_CHECK(hipGetLastError());
}

// n ASCII queries of L bytes each, back to back: counts (and status) only.  Nucleotide: packed on the device and served by
// the packed kernels.  Amino k-mers with a seed table: the two-phase schedule (count_aa_kmer_probe_kernel, then the
// generic kernel on what it listed).  Anything else: the generic kernel reading its queries at q * L.
// d_ranges (optional): (start, end) / RS_* words per query for the locate pass, as launch_count_ascii writes them.
void launch_count_ascii_uniform(Replica& r, const uint8_t* d_q, uint64_t n, uint64_t L, uint64_t* d_counts, uint8_t* d_status, hipStream_t s,
                                uint64_t* d_ranges = nullptr, unsigned long long* d_tally = nullptr) {
  if (n == 0) return;
  require(L >= 1, "query length must be at least 1");
  static const bool off = getenv("AWRY_AA_KMER") && !strcmp(getenv("AWRY_AA_KMER"), "0");
  static const bool no_long = getenv("AWRY_AA_LONG") && !strcmp(getenv("AWRY_AA_LONG"), "0");
  const bool two_phase = !off && r.dev.alphabet == AMINO && L >= (uint64_t)AA_KMER_MIN && L <= (uint64_t)(no_long ? AA_KMER_MAX : AA_KMER_LONG_MAX) &&
                         r.seed_k >= 1 && (uint64_t)r.seed_k <= L && n < (1ull << 32);
  const ScratchLock scratch_lock(r, s);
  Replica::SurvScratch* sc = surv_scratch(r, s);
  if (r.dev.alphabet == NUCLEOTIDE && !d_ranges && L <= 4096 && n < (1ull << 32)) {
    // the device half of the packed host path: pack 2 bits per letter, packed kernels, and the generic kernel over the
    // pack kernel's list for the queries with letters outside ACGT (it also writes their status)
    const uint64_t W = (L + 31) / 32;
    if (sc->u_words.n < n * W || sc->u_list.n < n || !sc->u_bad.p) {
      HIP_CHECK(hipStreamSynchronize(s));
      if (sc->u_words.n < n * W) sc->u_words.alloc(n * W + n * W / 4);
      if (sc->u_list.n < n) sc->u_list.alloc(n + n / 4);
      if (!sc->u_bad.p) sc->u_bad.alloc(2);
    }
    HIP_CHECK(hipMemsetAsync(sc->u_bad.p, 0, 16, s));
    if (d_status) HIP_CHECK(hipMemsetAsync(d_status, 0, n, s));
    launch_pack_nt2(r, d_q, nullptr, 0, n, n * L, (int)L, (int)W, sc->u_words.p, nullptr, sc->u_bad.p, s, sc->u_list.p);
    if (L <= 32) launch_count_nt2(r, sc->u_words.p, n, (int)L, d_counts, true, s, nullptr);
    else launch_count_nt2_long(r, sc->u_words.p, n, (int)L, d_counts, nullptr, true, s, nullptr);
    const QueryList ql{sc->u_list.p, nullptr, 0, sc->u_bad.p, nullptr, 0};
    hipLaunchKernelGGL((count_scalar_kernel<NUCLEOTIDE, LIST_GLOBAL>), dim3((unsigned)r.num_cus * 2), dim3(256), 0, s, r.dev, d_q, nullptr, n,
                       d_counts, nullptr, d_status, 1, L, ql);
    HIP_CHECK(hipGetLastError());
    return;
  }
  if (!two_phase) {
    require(!d_tally, "the census is kept by the amino k-mer schedule only");
    launch_count_ascii(r, d_q, nullptr, n, d_counts, d_ranges, d_status, s, true, L);
    return;
  }
  launch_aa_two_phase(r, d_q, nullptr, n, (int)L, d_counts, d_ranges, d_status, s, d_tally);
}

// Expansions (rank_all pairs) one pattern may take before its search is abandoned with Q_EXPANSION_CAP.  A safety bound for
// a shared card (DESIGN.md 5d has its basis).  Read per call: AWRY_PATTERN_MAX_EXPANSIONS (tests shrink it).
uint64_t pattern_max_expansions() {
  const char* e = getenv("AWRY_PATTERN_MAX_EXPANSIONS");
  const uint64_t v = e ? strtoull(e, nullptr, 10) : 0;
  return v ? v : (uint64_t)AWRY_PATTERN_DEFAULT_MAX_EXPANSIONS;
}

// the DFS kernel (mismatch_kernels.hip.h) on a resident grid (lanes draw queries from the work-queue head).  classes: the
// queries are class patterns; the frames a lane cannot keep in registers then live in the stream's scratch, sized to the
// grid, and the expansion cap applies -- the letter mode has neither.  EMIT: the locate pass that writes the leaves of query
// q to key / val [leaf_off[q], leaf_off[q + 1])
void launch_count_leaves(Replica& r, bool classes, const uint8_t* d_q, const uint64_t* d_off, uint64_t n, int k, uint64_t* d_counts,
                         uint64_t* d_totals, uint64_t* d_nleaves, uint8_t* d_status, hipStream_t s, unsigned long long* d_tally = nullptr,
                         const uint64_t* d_leaf_off = nullptr, uint64_t* d_key = nullptr, uint64_t* d_val = nullptr) {
  if (n == 0) return;
  // the class mode's workspace, and in both modes the work-queue head: its memset and the kernel are queued as one step
  const ScratchLock scratch_lock(r, s);
  unsigned long long* ctr = next_counter(r, s);
  const bool emit = d_leaf_off != nullptr;
  const uint64_t want = (n + 255) / 256, max_exp = classes ? pattern_max_expansions() : 0;
  with_alphabet(r.dev.alphabet, [&](auto A) {
    with_flags(classes, emit, [&](auto C, auto E) {
      auto kernel = count_dfs_kernel<decltype(A)::value, C(), E()>;  // (A is a capture here: its type names the value)
      const dim3 g((unsigned)std::max<uint64_t>(1, std::min<uint64_t>(want, resident_grid(r, kernel)))), b(256);
      uint64_t* ws = nullptr;
      if (C()) {
        Replica::SurvScratch* sc = surv_scratch(r, s);
        const size_t need = (size_t)PT_WS_WORDS * g.x * b.x;
        if (sc->pat_stack.n < need) {
          HIP_CHECK(hipStreamSynchronize(s));
          sc->pat_stack.alloc(need);
        }
        ws = sc->pat_stack.p;
      }
      hipLaunchKernelGGL(kernel, g, b, 0, s, r.dev, d_q, d_off, n, k, max_exp, d_counts, d_totals, d_nleaves, d_status, d_leaf_off, d_key, d_val, ws,
                         ctr, d_tally);
    });
  });
  HIP_CHECK(hipGetLastError());
}

// anchors (kernels_anchor.hip.h) on a resident grid.  d_anchor_off == nullptr: the count pass (d_n_anchors, d_status); else the
// fill pass, which writes the records of query q at d_anchors[d_anchor_off[q] ...) (d_n_anchors / d_status nullable there)
void launch_anchors(Replica& r, const uint8_t* d_q, const uint64_t* d_off, uint64_t n, uint32_t min_len, int skip, uint64_t* d_n_anchors,
                    const uint64_t* d_anchor_off, Anchor* d_anchors, uint8_t* d_status, hipStream_t s, unsigned long long* d_tally = nullptr) {
  if (n == 0) return;
  const uint64_t want = (n + 255) / 256;
  with_alphabet(r.dev.alphabet, [&](auto A) {
    with_flags(d_anchor_off != nullptr, [&](auto F) {
      auto kernel = anchor_scalar_kernel<decltype(A)::value, F() ? 1 : 0>;
      const dim3 g((unsigned)std::max<uint64_t>(1, std::min<uint64_t>(want, resident_grid(r, kernel)))), b(256);
      hipLaunchKernelGGL(kernel, g, b, 0, s, r.dev, d_q, d_off, n, min_len, (uint32_t)skip, d_n_anchors, d_anchor_off, d_anchors, d_status, d_tally);
    });
  });
  HIP_CHECK(hipGetLastError());
}

// SMEMs (kernels_smem.hip.h) on a resident grid, with launch_anchors' two passes.  The forward form is the replica's: the
// suffix-array search where the dense SA at ratio 1 and text8 are resident, else bisection over backward searches.
bool smem_sa_form(const Replica& r) { return r.dev.dense_sa && r.dev.dense_ratio == 1 && r.dev.text8; }
void launch_smems(Replica& r, const uint8_t* d_q, const uint64_t* d_off, uint64_t n, uint32_t min_len, uint64_t* d_n_smems, const uint64_t* d_smem_off,
                  Anchor* d_smems, uint8_t* d_status, hipStream_t s, unsigned long long* d_tally = nullptr) {
  if (n == 0) return;
  const uint64_t want = (n + 255) / 256;
  with_alphabet(r.dev.alphabet, [&](auto A) {
    with_flags(smem_sa_form(r), d_smem_off != nullptr, [&](auto SA, auto F) {
      auto kernel = smem_scalar_kernel<decltype(A)::value, SA() ? SMEM_FWD_SA : SMEM_FWD_LF, F() ? 1 : 0>;
      const dim3 g((unsigned)std::max<uint64_t>(1, std::min<uint64_t>(want, resident_grid(r, kernel)))), b(256);
      hipLaunchKernelGGL(kernel, g, b, 0, s, r.dev, d_q, d_off, n, min_len, d_n_smems, d_smem_off, d_smems, d_status, d_tally);
    });
  });
  HIP_CHECK(hipGetLastError());
}

// The edit scan (edit_kernels.hip.h) over m windows, one per lane.  d_hit_off == nullptr: the count pass (d_n_hits[m]); else the
// fill pass (d_gpos / d_edits at [d_hit_off[w], d_hit_off[w + 1])).  W = words of 64 query letters per column, for the launch:
// the chunk's longest query decides it (a shorter query leaves its upper words idle); nqueries != 0: the windows' queries are
// 0 .. nqueries - 1 and the pattern masks are built per query; nqueries == 0 (the device entry point, which knows neither the
// number of queries nor their lengths on the host): per window, at W = 4.  The masks live in the stream's scratch and are
// rebuilt by every launch, in front of the scan: two host threads on one stream never read each other's.
void launch_edit_windows(Replica& r, const uint8_t* text8, const uint8_t* d_q, const uint64_t* d_off, const uint32_t* d_win_query,
                         const uint64_t* d_win_first, const uint32_t* d_win_count, uint64_t m, int k, int W, uint64_t nqueries, uint64_t* d_n_hits,
                         const uint64_t* d_hit_off, uint64_t* d_gpos, uint8_t* d_edits, hipStream_t s, unsigned long long* d_tally = nullptr) {
  if (m == 0) return;
  require(W >= 1 && W <= EDIT_MAX_W, "internal: words per column out of range");
  const ScratchLock scratch_lock(r, s);
  Replica::SurvScratch* sc = surv_scratch(r, s);
  const uint64_t nslots = nqueries ? nqueries : m;
  const size_t need = (size_t)nslots * (size_t)edit_symbols(r.dev.alphabet) * (size_t)W;
  if (sc->edit_masks.n < need) {
    HIP_CHECK(hipStreamSynchronize(s));
    sc->edit_masks.alloc(need + need / 4);
  }
  const bool fill = d_hit_off != nullptr;
  with_alphabet(r.dev.alphabet, [&](auto A) {
    constexpr int AL = decltype(A)::value;
    hipLaunchKernelGGL(edit_masks_kernel<AL>, dim3(grid_for(r, need, 256)), dim3(256), 0, s, d_q, d_off, nqueries ? nullptr : d_win_query, nslots, W,
                       sc->edit_masks.p);
    const dim3 g(grid_for(r, m, 256)), b(256);
    auto scan = [&](auto WW, auto F) {
      hipLaunchKernelGGL((edit_scan_kernel<AL, decltype(WW)::value, decltype(F)::value>), g, b, 0, s, text8, r.dev.bwt_len - 1, d_off, d_win_query,
                         d_win_first, d_win_count, m, k, sc->edit_masks.p, nqueries ? 0 : 1, d_n_hits, d_hit_off, d_gpos, d_edits, d_tally);
    };
    with_flags(fill, [&](auto F) {
      switch (W) {
        case 1: scan(std::integral_constant<int, 1>{}, F); break;
        case 2: scan(std::integral_constant<int, 2>{}, F); break;
        case 3: scan(std::integral_constant<int, 3>{}, F); break;
        default: scan(std::integral_constant<int, 4>{}, F); break;
      }
    });
  });
  HIP_CHECK(hipGetLastError());
}

// The alignment pass (kernels_align.hip.h) over m hits, one per lane: text_len[m], n_ops[m] and ops[m * ALIGN_MAX_OPS].  The band
// half-width of the launch is the smallest of 2, 4, 6, 8 that holds k; max_rows = the longest query the launch takes (the chunk's
// longest, or EDIT_MAX_LEN for the device entry point).  The direction words live in the stream's scratch, one per row and grid
// lane: the grid is cut so that they stay within ALIGN_TRACE_BYTES (at 256 rows and 8-byte words 256 blocks: one per CU).
constexpr size_t ALIGN_TRACE_BYTES = 128u << 20;
void launch_edit_align(Replica& r, const uint8_t* text8, const uint8_t* d_q, const uint64_t* d_off, const uint32_t* d_hit_query,
                       const uint64_t* d_hit_gpos, const uint8_t* d_hit_edits, uint64_t m, int k, uint32_t max_rows, uint32_t* d_text_len, uint8_t* d_n_ops,
                       uint32_t* d_ops, hipStream_t s, unsigned long long* d_tally = nullptr) {
  if (m == 0) return;
  require(max_rows >= 1 && max_rows <= (uint32_t)EDIT_MAX_LEN && k >= 0 && k <= EDIT_MAX_K, "internal: alignment launch out of range");
  const ScratchLock scratch_lock(r, s);
  Replica::SurvScratch* sc = surv_scratch(r, s);
  with_alphabet(r.dev.alphabet, [&](auto A) {
    constexpr int AL = decltype(A)::value;
    auto align = [&](auto HH) {
      constexpr int H = decltype(HH)::value;
      using TW = typename AlignTrace<H>::word;
      const uint64_t fit = ALIGN_TRACE_BYTES / ((size_t)max_rows * sizeof(TW) * 256);
      const uint64_t blocks = std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)grid_for(r, m, 256), fit));
      const size_t need = ((size_t)blocks * 256 * max_rows * sizeof(TW) + 7) / 8;
      if (sc->align_trace.n < need) {
        HIP_CHECK(hipStreamSynchronize(s));
        sc->align_trace.alloc(need);
      }
      hipLaunchKernelGGL((edit_align_kernel<AL, H>), dim3((unsigned)blocks), dim3(256), 0, s, text8, r.dev.bwt_len - 1, d_q, d_off, d_hit_query, d_hit_gpos,
                         d_hit_edits, m, k, max_rows, reinterpret_cast<TW*>(sc->align_trace.p), d_text_len, d_n_ops, d_ops, d_tally);
    };
    if (k <= 2) align(std::integral_constant<int, 2>{});
    else if (k <= 4) align(std::integral_constant<int, 4>{});
    else if (k <= 6) align(std::integral_constant<int, 6>{});
    else align(std::integral_constant<int, 8>{});
  });
  HIP_CHECK(hipGetLastError());
}

// Chaining (kernels_chain.hip.h) on n queries' seeds.  d_chain_off == nullptr: the count pass (d_n_chains, d_n_members); else the
// fill pass.  A group of 16 lanes owns a query when lookback <= 16, else a wave (AWRY_CHAIN_GROUP=64, read per call: the wave there
// too).  Queries beyond the group's LDS tile work in a slab of the stream's scratch, one per group of the grid: the grid is cut so
// that the slabs stay within CHAIN_SLAB_BYTES (at max_seeds = 4096, 144 KiB a slab: 910 groups).
constexpr size_t CHAIN_SLAB_BYTES = 128u << 20;
int chain_group_width(uint32_t lookback) {
  const char* e = getenv("AWRY_CHAIN_GROUP");
  return lookback <= 16 && !(e && atoi(e) == 64) ? 16 : 64;
}
void launch_chain(Replica& r, const uint64_t* d_seed_off, const Seed* d_seeds, uint64_t n, const ChainParams& P, uint64_t* d_n_chains,
                  uint64_t* d_n_members, const uint64_t* d_chain_off, const uint64_t* d_member_off, Chain* d_chains, Seed* d_members, uint8_t* d_status,
                  hipStream_t s, unsigned long long* d_tally = nullptr) {
  if (n == 0) return;
  const ScratchLock scratch_lock(r, s);
  Replica::SurvScratch* sc = surv_scratch(r, s);
  auto chain = [&](auto GG, auto F) {
    constexpr int G = decltype(GG)::value, GROUPS = 256 / G;
    uint32_t slab_cap = 0;
    if (P.max_seeds > (uint32_t)ChainTile<G>::value)
      for (slab_cap = 1; slab_cap < P.max_seeds;) slab_cap <<= 1;
    uint64_t blocks = (uint64_t)grid_for(r, n, GROUPS, 4);
    const size_t slab = (size_t)slab_cap * CHAIN_SEED_BYTES * GROUPS;  // per block
    if (slab) blocks = std::max<uint64_t>(1, std::min<uint64_t>(blocks, CHAIN_SLAB_BYTES / slab));
    if (sc->chain_slabs.n < blocks * slab) {
      HIP_CHECK(hipStreamSynchronize(s));
      sc->chain_slabs.alloc(blocks * slab);
    }
    hipLaunchKernelGGL((chain_kernel<G, decltype(F)::value ? 1 : 0>), dim3((unsigned)blocks), dim3(256), 0, s, r.dev, d_seed_off, d_seeds, n, P, d_n_chains,
                       d_n_members, d_chain_off, d_member_off, d_chains, d_members, d_status, reinterpret_cast<char*>(sc->chain_slabs.p), slab_cap, d_tally);
  };
  with_flags(d_chain_off != nullptr, [&](auto F) {
    if (chain_group_width(P.lookback) == 16) chain(std::integral_constant<int, 16>{}, F);
    else chain(std::integral_constant<int, 64>{}, F);
  });
  HIP_CHECK(hipGetLastError());
}

// Chain alignment (kernels_chain_align.hip.h) over m chains.  d_cigar_off == nullptr: the count pass (d_alns, d_n_ops); else the
// fill pass.  Each pass classifies the chains anew (class lists in the stream's scratch: 3 m + 3 words) and runs the three
// instantiations one after the other, each over its list; a launch whose list is empty ends at once.  The direction words live
// in the stream's align_trace, max_rows (the longest query the launch takes) * 4, 8 or 16 bytes per grid lane: the grid of each
// class is cut so that they stay within CHAIN_ALIGN_TRACE_BYTES (at 1024 rows: 512, 256 and 128 blocks of 256 lanes; at the 101 rows
// of a short-read batch the whole grid), and the scratch grows to what the launch needs, not to the bound.
constexpr size_t CHAIN_ALIGN_TRACE_BYTES = 512u << 20;
// md: end to end (d_alns: Aln records) or clipped (AlnClip records): the same kernels, instantiated per mode.
void launch_chain_align(Replica& r, const uint8_t* text8, const uint8_t* d_q, const uint64_t* d_off, const uint32_t* d_chain_query,
                        const uint64_t* d_member_off, const Seed* d_members, uint64_t m, int band, const AlignMode& md, uint32_t max_rows, void* d_alns,
                        uint64_t* d_n_ops, const uint64_t* d_cigar_off, uint32_t* d_cigar, hipStream_t s, unsigned long long* d_tally = nullptr) {
  if (m == 0) return;
  require(m < (1ull << 32), "more than 2^32 - 1 chains in one alignment launch");
  require(max_rows >= 1 && max_rows <= (uint32_t)CHAIN_ALIGN_MAX_LEN && band >= 0 && band <= CHAIN_ALIGN_MAX_BAND,
          "internal: chain alignment launch out of range");
  const ScratchLock scratch_lock(r, s);
  Replica::SurvScratch* sc = surv_scratch(r, s);
  const size_t lists_need = (size_t)CHAIN_ALIGN_CLASSES * m + CHAIN_ALIGN_CLASSES;
  auto blocks_for = [&](size_t row_bytes) {
    return std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)grid_for(r, m, 256), CHAIN_ALIGN_TRACE_BYTES / ((size_t)max_rows * row_bytes * 256)));
  };
  size_t trace_bytes = 0;
  for (int cls = 0; cls < CHAIN_ALIGN_CLASSES; cls++) {
    const size_t row_bytes = (size_t)4 << cls;  // ChainAlignTrace: NW * sizeof(word) = 4, 8, 16
    trace_bytes = std::max(trace_bytes, (size_t)blocks_for(row_bytes) * 256 * max_rows * row_bytes);
  }
  const size_t trace_need = (trace_bytes + 7) / 8;
  if (sc->chain_align_lists.n < lists_need || sc->align_trace.n < trace_need) {
    HIP_CHECK(hipStreamSynchronize(s));
    if (sc->chain_align_lists.n < lists_need) sc->chain_align_lists.alloc(lists_need + lists_need / 4);
    if (sc->align_trace.n < trace_need) sc->align_trace.alloc(trace_need);
  }
  uint32_t* lists = sc->chain_align_lists.p;
  uint32_t* list_n = lists + (size_t)CHAIN_ALIGN_CLASSES * m;
  HIP_CHECK(hipMemsetAsync(list_n, 0, CHAIN_ALIGN_CLASSES * sizeof(uint32_t), s));
  const bool fill = d_cigar_off != nullptr;
  with_flags(md.clip, [&](auto M) {
    constexpr bool CLIP = decltype(M)::value;
    AlnOf<CLIP>* alns = static_cast<AlnOf<CLIP>*>(d_alns);
    hipLaunchKernelGGL(chain_align_classify_kernel<CLIP>, dim3(grid_for(r, m, 256)), dim3(256), 0, s, r.dev.bwt_len - 1, d_off, d_chain_query, d_member_off,
                       d_members, m, band, max_rows, fill ? nullptr : alns, fill ? nullptr : d_n_ops, lists, list_n);
    with_alphabet(r.dev.alphabet, [&](auto A) {
      constexpr int AL = decltype(A)::value;
      with_flags(fill, [&](auto F) {
        auto align = [&](auto CC) {
          constexpr int CLS = decltype(CC)::value, NBMAX = chain_align_class_nb(CLS);
          using TR = ChainAlignTrace<NBMAX>;
          using TW = typename TR::word;
          static_assert(TR::NW * sizeof(TW) == ((size_t)4 << CLS), "the trace bytes per row of the class");
          const uint64_t blocks = blocks_for(TR::NW * sizeof(TW));
          hipLaunchKernelGGL((chain_align_kernel<AL, NBMAX, decltype(F)::value, CLIP>), dim3((unsigned)blocks), dim3(256), 0, s, text8, r.dev.bwt_len - 1, d_q,
                             d_off, d_chain_query, d_member_off, d_members, lists + (size_t)CLS * m, list_n + CLS, band, reinterpret_cast<TW*>(sc->align_trace.p),
                             alns, d_n_ops, d_cigar_off, d_cigar, d_tally, r.dev, md);
        };
        if (2 * band + 1 <= chain_align_class_nb(0)) align(std::integral_constant<int, 0>{});
        if (2 * band + 1 <= chain_align_class_nb(1)) align(std::integral_constant<int, 1>{});
        align(std::integral_constant<int, 2>{});
      });
    });
  });
  HIP_CHECK(hipGetLastError());
}

// The doubled batch of n reads (kernels_map.hip.h): d_out_bytes holds 2 (d_off[n] - d_off[0]) bytes, d_out_off 2 n + 1 offsets.
void launch_strand_expand(Replica& r, const uint8_t* d_q, const uint64_t* d_off, uint64_t n, uint8_t* d_out_bytes, uint64_t* d_out_off, hipStream_t s) {
  require(r.dev.alphabet == NUCLEOTIDE, "the reverse complement needs a nucleotide index");
  if (n == 0) { HIP_CHECK(hipMemsetAsync(d_out_off, 0, 8, s)); return; }
  hipLaunchKernelGGL(strand_expand_kernel, dim3(grid_for(r, n * MAP_EXPAND_GROUP, 256)), dim3(256), 0, s, d_q, d_off, n, d_out_bytes, d_out_off);
  HIP_CHECK(hipGetLastError());
}

// Rank, redundancy, report and MAPQ over the alignment records of a doubled batch of n reads (kernels_map.hip.h).  d_map_off ==
// nullptr: the count pass (d_n_maps, d_read_status nullable); else the fill pass (d_maps; d_sel, d_pos nullable).
// md: end to end (Aln in, MapRec out) or clipped (AlnClip in, MapClipRec out): the same kernel, instantiated per mode.
void launch_map_select(Replica& r, const uint64_t* d_aln_off, const void* d_alns, const Chain* d_chains, const uint8_t* d_chain_status, uint64_t n,
                       uint32_t chains_per_strand, uint32_t max_report, const MapMode& md, uint64_t* d_n_maps, uint8_t* d_read_status,
                       const uint64_t* d_map_off, void* d_maps, uint32_t* d_sel, uint64_t* d_pos, hipStream_t s) {
  if (n == 0) return;
  with_flags(d_map_off != nullptr, md.clip, [&](auto F, auto M) {
    constexpr bool CLIP = decltype(M)::value;
    hipLaunchKernelGGL((map_select_kernel<F(), CLIP>), dim3(grid_for(r, n, 256)), dim3(256), 0, s, r.dev, d_aln_off, static_cast<const AlnOf<CLIP>*>(d_alns),
                       d_chains, d_chain_status, n, chains_per_strand, max_report, d_n_maps, d_read_status, d_map_off, static_cast<MapRecOf<CLIP>*>(d_maps),
                       d_sel, d_pos, md);
  });
  HIP_CHECK(hipGetLastError());
}

// The split selection over the clipped alignment records of a doubled batch of n reads (kernels_split.hip.h): launch_map_select's
// protocol and outputs with MapSplitRec records.  qstride: 1 when d_qoff holds the reads' own n + 1 offsets, 2 when it holds the
// doubled batch's 2 n + 1; only the lengths are read.
void launch_map_split_select(Replica& r, const uint64_t* d_aln_off, const AlnClip* d_alns, const Chain* d_chains, const uint8_t* d_chain_status,
                             const uint64_t* d_qoff, uint32_t qstride, uint64_t n, uint32_t chains_per_strand, const SplitParams& sp, const MapMode& md,
                             uint64_t* d_n_maps, uint8_t* d_read_status, const uint64_t* d_map_off, MapSplitRec* d_maps, uint32_t* d_sel, uint64_t* d_pos,
                             hipStream_t s) {
  if (n == 0) return;
  require(md.clip, "internal: the split selection reads clipped records");
  with_flags(d_map_off != nullptr, [&](auto F) {
    hipLaunchKernelGGL((map_split_select_kernel<F()>), dim3(grid_for(r, n, 256)), dim3(256), 0, s, r.dev, d_aln_off, d_alns, d_chains, d_chain_status, d_qoff,
                       qstride, n, chains_per_strand, sp, d_n_maps, d_read_status, d_map_off, d_maps, d_sel, d_pos, md);
  });
  HIP_CHECK(hipGetLastError());
}

// The rescue windows of P pairs (kernels_pair.hip.h): 2 P rescue_anchors slots at a fixed stride.  qstride: 1 when d_qoff holds the
// reads' own 2 P + 1 offsets, 2 when it holds the doubled batch's.  Rec: MapRec end to end, MapClipRec in the clipped mode.
template <class Rec>
void launch_pair_windows(Replica& r, const uint64_t* d_cand_off, const Rec* d_cands, const uint64_t* d_qoff, uint32_t qstride, uint64_t P,
                         const PairParams& pp, uint32_t* d_win_query, uint64_t* d_win_first, uint32_t* d_win_count, hipStream_t s) {
  const uint64_t slots = 2 * P * pp.rescue_anchors;
  if (slots == 0) return;
  hipLaunchKernelGGL(pair_windows_kernel<Rec>, dim3(grid_for(r, slots, 256)), dim3(256), 0, s, r.dev, d_cand_off, d_cands, d_qoff, qstride, P, pp, d_win_query,
                     d_win_first, d_win_count);
  HIP_CHECK(hipGetLastError());
}

// Pair choice over the kept lists and the rescued candidates of P pairs (kernels_pair.hip.h).  d_map_off == nullptr: the count pass
// (d_n_maps[2 P]); else the fill pass (d_maps; d_sel, d_pos, d_insert nullable).  d_resc == nullptr: no rescued candidates.
// Rec and md: MapRec end to end, MapClipRec with the clipped mode's scalars.
template <class Rec>
void launch_pair_select(Replica& r, const uint64_t* d_cand_off, const Rec* d_cands, const Rec* d_resc, const uint8_t* d_read_status, uint64_t P,
                        const PairParams& pp, const PairMode& md, uint64_t* d_n_maps, const uint64_t* d_map_off, Rec* d_maps, uint32_t* d_sel,
                        uint64_t* d_pos, uint32_t* d_insert, hipStream_t s) {
  if (P == 0) return;
  require(md.clip == pair_clipped<Rec>, "internal: the pair records are not the mode's");
  with_flags(d_map_off != nullptr, [&](auto F) {
    hipLaunchKernelGGL((pair_select_kernel<F(), Rec>), dim3(grid_for(r, P, 256)), dim3(256), 0, s, r.dev, d_cand_off, d_cands, d_resc, d_read_status, P, pp,
                       d_n_maps, d_map_off, d_maps, d_sel, d_pos, d_insert, md);
  });
  HIP_CHECK(hipGetLastError());
}

// anchor records -> (start_row, end_row) pairs and located counts (0 for anchors of more than max_hits rows)
void launch_anchor_ranges(Replica& r, const Anchor* d_anchors, uint64_t n, uint64_t max_hits, uint64_t* d_ranges, uint64_t* d_located, hipStream_t s) {
  if (n == 0) return;
  hipLaunchKernelGGL(anchor_ranges_kernel, dim3(grid_for(r, n, 256)), dim3(256), 0, s, d_anchors, n, max_hits, d_ranges, d_located);
  HIP_CHECK(hipGetLastError());
}

}  // namespace
