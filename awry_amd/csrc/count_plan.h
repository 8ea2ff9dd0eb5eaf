// count_plan.h -- which schedule a launch of packed nucleotide queries takes, as a pure function of what the replica holds
// Plain C++ (no HIP): launch_count_nt2 / launch_count_nt2_long (launchers.h) switch on the plan, awry_count_schedule names
// it, prewarm.h sizes scratch for its grids, and tests/test_count_plan_cpu.py compiles it on its own.  DESIGN.md, "The count plan".
#pragma once
#include <stdint.h>

#include "layout.h"  // NUCLEOTIDE, LIST_MAX_LISTS, LCX_LF_CHUNK

namespace awry {

// k-mers shorter than the seed table's k: a complete table of their own length ("rung", accelerators.h seed_rung), for
// lengths SEED_RUNG_MIN .. SEED_RUNG_MAX (shorter k-mers: a handful of LF steps over blocks that live in L2; longer: 4^L
// entries do not pay) and batches of SEED_RUNG_MIN_BATCH queries and more
constexpr int SEED_RUNG_MIN = 6, SEED_RUNG_MAX = 16;
constexpr uint64_t SEED_RUNG_MIN_BATCH = 4096;
// the k-mer count table (accelerators.h kmer_table) under policy: batches of this many queries and more
constexpr uint64_t KMER_TABLE_MIN_BATCH = 65536;

// What the policy reads (launchers.h count_facts fills it from a Replica).
struct CountFacts {
  int alphabet = NUCLEOTIDE;
  bool wide = false;  // 64-bit rows
  uint64_t bwt_len = 0;
  int seed_k = 0;
  bool seed = false, seed64 = false;  // the seed table (32-bit / wide entries) is resident
  bool text4 = false;                 // seed-and-verify: the 4-bit text ...
  uint32_t dense_ratio = 0;           // ... and the dense SA (at ratio 1)
  bool lcx_key = false;               // the left-context index is resident
  int kt_mode = -1;                   // awry_set_kmer_table: -1 policy, 0 never, 1 whatever the batch
  bool verify_kmers = false;          // awry_set_verify_kmers
  int num_cus = 0;
  int probe_resume_per_cu[4] = {8, 8, 8, 8};  // Replica::probe_resume_per_cu, by [2 * TALLY + VERIFY]
  unsigned lcx_reads_grid[2] = {0, 0};        // Replica::lcx_reads_grid, by [RAGGED]
  // awry_debug_set_count_kernel / AWRY_COUNT_KERNEL: 0 strided quads, 1 LDS-staged chunks, 2 groups of four, 3 two-phase,
  // 4 two-phase with the k-mer probe and resume passes as two launches on num_cus * 8 blocks (the schedule before the one
  // launch), 5 the same two launches on the one launch's grid (for A/B of fusion and grid size; the read and wide-row
  // schedules treat 4, 5 as 3); -1: no explicit choice (the policy below)
  int forced = -1;
  bool rungs_off = false, table_off = false;  // AWRY_SEED_RUNGS=0, AWRY_KMER_TABLE=0
  // both accelerators are built on first use and may not fit: the launcher then plans again with the fact set
  bool rung_failed = false, table_failed = false;
};

enum class CountSchedule {
  STRIDED_QUADS,      // count_nt2_quad_kernel
  LDS_CHUNKS,         // count_nt2_chunk_kernel
  QUAD4,              // count_nt2_quad4_kernel: groups of 4 consecutive queries per quad
  PROBE_RESUME,       // count_nt2_probe_resume_kernel: the two-phase k-mer schedule as one launch
  PROBE_THEN_RESUME,  // count_nt2_probe_kernel, count_nt2_resume_kernel
  READS_SINGLE,       // count_nt2_reads_kernel
  READS_LISTS,        // count_nt2_reads_probe_kernel, count_nt2_reads_kernel over the blocks' lists
  READS_LANES,        // count_nt2_reads_probe_kernel, lcx_quad_reads_kernel, count_nt2_reads_pool_kernel
  WIDE_SINGLE,        // count_nt2_wide_kernel
  WIDE_TWO_PHASE,     // count_nt2_wide_probe_kernel, count_nt2_wide_kernel over the blocks' lists
};

struct CountPlan {
  CountSchedule schedule = CountSchedule::STRIDED_QUADS;
  // template arguments of the kernels: SEEDED and VERIFY where the schedule's kernels have them (false elsewhere)
  bool seeded = false, verify = false;
  bool rung = false;   // the launch takes the rung table of its length (built on first use)
  bool table = false;  // the launch takes the k-mer count table of its length (built on first use)
  // the grid: `blocks` for every launch of the schedule but the lane pass (also the number of survivor lists), or, with
  // blocks == 0, sized from the batch: grid_for(n * items_per_query, 256)
  unsigned blocks = 0, items_per_query = 0;
  unsigned lcx_grid = 0;  // READS_LANES: blocks of lcx_quad_reads_kernel
};

// slots of one survivor list of a two-phase launch over n queries on nblk blocks: the queries a block sees, ceil(n / (nblk * 256)) * 256
inline uint64_t list_slots_per_block(uint64_t n, unsigned nblk) { return ((n + (uint64_t)nblk * 256 - 1) / ((uint64_t)nblk * 256)) * 256; }

// The LF list lcx_quad_reads_kernel appends to on a grid of `grid` blocks (4 waves each), for `total` list slots of survivors.
// A wave reserves LCX_LF_CHUNK slots at a time with one atomic and fills them in order.  One append is one item per quad
// (16 per wave at most), and the wave reserves its next chunk only when an append does not fit in what is left, so every
// chunk it leaves behind holds more than LCX_LF_CHUNK - 16 items; the chunk a wave holds at its end may be almost empty.
// A wave that reserves c chunks thus appends at least (c - 1) (LCX_LF_CHUNK - 15) items, and the waves append at most
// `total` items in all (each survivor at most once):
//   sum_w (c_w - 1) <= floor(total / (LCX_LF_CHUNK - 15)),   chunks <= that + nwaves,
//   slots = LCX_LF_CHUNK * chunks <= total + 15 * ceil(total / (LCX_LF_CHUNK - 15)) + nwaves * LCX_LF_CHUNK.
inline uint64_t lcx_lf_list_bound(uint64_t total, unsigned grid) {
  const uint64_t per = (uint64_t)LCX_LF_CHUNK - 15, nwaves = 4ull * grid;
  return total + (total + per - 1) / per * 15 + nwaves * (uint64_t)LCX_LF_CHUNK;
}

namespace count_plan_detail {

constexpr uint64_t U32_ROWS = 1ull << 32;  // the two-phase schedules number their queries with u32

// seed-and-verify has its accelerators (the 4-bit text, the dense SA at ratio 1)
inline bool verify_resident(const CountFacts& f) { return f.text4 && f.dense_ratio == 1; }
inline bool two_phase_forced(const CountFacts& f) { return f.forced >= 3 && f.forced <= 5; }
inline CountPlan sized_from_n(CountPlan p, CountSchedule s, unsigned items_per_query) {
  p.schedule = s;
  p.items_per_query = items_per_query;
  return p;
}

// Wide-row replicas (64-bit rows), k-mers and reads: the two-phase schedule (count_nt2_wide_probe_kernel + the listed quad
// pass) is an alternative, not the policy -- on a GRCh38-scale index forced onto 64-bit rows (k = 16, 69 GB of 16-byte
// entries) it runs random 31-mers at 16.7 against 16.5 G/s and reads from the text 10 % slower than the single strided quad
// kernel: without the 32-bit accelerators (dense SA, text, position seeds) the entry settles too few queries for a second
// launch to pay.  Selected with AWRY_COUNT_KERNEL=twophase / awry_debug_set_count_kernel(3).
inline CountPlan plan_wide(const CountFacts& f, uint64_t n, int L, bool use_seed, bool ragged) {
  CountPlan p;
  p.seeded = use_seed && f.seed_k > 0 && f.seed64 && (ragged || f.seed_k <= L);  // ragged reads decide per read
  if (!(p.seeded && two_phase_forced(f) && n < U32_ROWS)) return sized_from_n(p, CountSchedule::WIDE_SINGLE, 4);
  p.schedule = CountSchedule::WIDE_TWO_PHASE;  // per-lane probe pass, then the quads on what has to be stepped
  p.blocks = (unsigned)f.num_cus * 8;
  return p;
}

}  // namespace count_plan_detail

// n packed k-mers of L <= 32 letters (launch_count_nt2); tally: the launch keeps the work census
inline CountPlan plan_kmers(const CountFacts& f, uint64_t n, int L, bool use_seed, bool tally) {
  using namespace count_plan_detail;
  if (f.wide) return plan_wide(f, n, L, use_seed, false);  // one word per k-mer is the W = 1 case of the wide kernel
  CountPlan p;
  // k-mers shorter than the seed table's k: their own complete table -- the entry IS the answer, where LF steps from the
  // last letter cost L dependent block reads (GRCh38 scale: 12-mers 5.6 -> 30+ G/s)
  p.rung = use_seed && f.seed_k > L && f.seed && n >= SEED_RUNG_MIN_BATCH && n < U32_ROWS && f.forced < 0 && !f.rungs_off &&
           f.alphabet == NUCLEOTIDE && L >= SEED_RUNG_MIN && L <= SEED_RUNG_MAX && !f.rung_failed;
  p.seeded = p.rung || (use_seed && f.seed_k > 0 && f.seed_k <= L);
  // Policy, from measurements on MI355X, GRCh38-scale, 10 M random 31-mers per launch (tools/ab_count.py, G queries/s):
  //   seed k   strided  quad4  chunk  twophase
  //     14      10.1    10.3    9.9     8.2
  //     16      19.4    21.8   14.4    21.3
  //     17      25.3    28.1     -     29.9
  // quad4 is the general default; once the table is so sparse that most queries are decided by their entry alone
  // (4^k >= 3 bwt_len) the per-lane probe pass of the two-phase schedule wins.
  // The LDS-staged variant (forced only) is equal at seed k=14 and 23% slower at k=16: the strided kernel's query words
  // already arrive as L2 hits, so staging only removes the partial-line result writes and pays chunk drain + refill for it.
  const bool sparse = p.seeded && f.seed_k >= 1 && f.seed_k <= 31 && (1ull << (2 * f.seed_k)) / 3 >= f.bwt_len;
  const int mode = p.rung ? 3 : f.forced >= 0 ? f.forced : sparse ? 3 : 2;
  if (mode == 1) return sized_from_n(p, CountSchedule::LDS_CHUNKS, 4);
  if (mode >= 3 && mode <= 5 && p.seeded && n < U32_ROWS) {
    // two-phase: per-lane seed probes decide most queries, the quad machinery resumes the survivors -- in one launch on
    // the resident grid, or (modes 4 and 5, for A/B) as the probe and resume kernels on num_cus * 8 blocks / that grid.
    // Survivors of phase 1 use seed-and-verify whenever its accelerators are resident (cheap: random batches barely
    // reach phase 2); the single-kernel schedules use it only on request (awry_set_verify_kmers)
    p.schedule = mode == 3 ? CountSchedule::PROBE_RESUME : CountSchedule::PROBE_THEN_RESUME;
    p.verify = verify_resident(f);
    p.blocks = (unsigned)f.num_cus * (mode == 4 ? 8u : (unsigned)f.probe_resume_per_cu[2 * tally + p.verify]);
    // survivors with a bucket of the left-context index: the count table of this length answers them from one line.  The
    // policy: batches of KMER_TABLE_MIN_BATCH queries and more with no schedule forced -- small batches and forced schedules
    // keep the searches whose census the tests of those schedules read.  awry_set_kmer_table(1): whatever the batch; (0): never.
    p.table = mode == 3 && p.verify && !p.rung && f.lcx_key && L > f.seed_k && !f.table_off && f.kt_mode != 0 &&
              (f.kt_mode == 1 || (n >= KMER_TABLE_MIN_BATCH && f.forced < 0)) && !f.table_failed;
    return p;
  }
  if (mode >= 2 && mode <= 5) {  // groups of 4 consecutive queries per quad: whole-sector result writes
    p.verify = f.verify_kmers && verify_resident(f);
    return sized_from_n(p, CountSchedule::QUAD4, 1);
  }
  return sized_from_n(p, CountSchedule::STRIDED_QUADS, 4);  // (mode 0, and any other number forced)
}

// n packed reads of L letters, or with `ragged` of up to L letters each (launch_count_nt2_long)
inline CountPlan plan_reads(const CountFacts& f, uint64_t n, int L, bool use_seed, bool ragged) {
  using namespace count_plan_detail;
  if (f.wide) return plan_wide(f, n, L, use_seed, ragged);
  CountPlan p;
  p.seeded = use_seed && f.seed_k > 0 && (ragged || f.seed_k <= L);  // ragged reads decide per read
  p.verify = verify_resident(f);
  if (!(p.verify && p.seeded && L - f.seed_k >= 3 && L <= 512 && n < U32_ROWS && (f.forced < 0 || two_phase_forced(f))))
    return sized_from_n(p, CountSchedule::READS_SINGLE, 4);
  // two-phase: a per-lane pass settles the reads their seed entry (plus one SA read and one text window) decides, the
  // quad code works through the rest: as a pooled search pass (lcx_quad_reads_kernel) + LF pass whenever the left-context
  // index is resident, else block b works through block b's list.  The pooled pass holds the prefix sums of the lists in
  // LDS and numbers the slots of its LF list with u32: it is taken only while both fit.
  p.blocks = (unsigned)f.num_cus * 8;
  const unsigned gl = f.lcx_reads_grid[ragged];
  const bool lanes = f.lcx_key && gl > 0 && p.blocks <= (unsigned)LIST_MAX_LISTS &&
                     lcx_lf_list_bound(list_slots_per_block(n, p.blocks) * p.blocks, gl) <= 0xFFFFFFFFull;
  p.schedule = lanes ? CountSchedule::READS_LANES : CountSchedule::READS_LISTS;
  p.lcx_grid = lanes ? gl : 0;
  return p;
}

// the kernels of the schedule, in launch order (awry_count_schedule)
inline const char* plan_name(const CountPlan& p) {
  switch (p.schedule) {
    case CountSchedule::STRIDED_QUADS: return "count_nt2_quad_kernel";
    case CountSchedule::LDS_CHUNKS: return "count_nt2_chunk_kernel";
    case CountSchedule::QUAD4: return "count_nt2_quad4_kernel";
    case CountSchedule::PROBE_RESUME:
      if (p.rung) return "count_nt2_probe_resume_kernel (table of its own for this length; batches of 4096 queries and more)";
      if (p.table)
        return "count_nt2_probe_resume_kernel (k-mer count table of this length: on first use with awry_set_kmer_table(1), else for batches of 65536 queries and more)";
      return "count_nt2_probe_resume_kernel";
    case CountSchedule::PROBE_THEN_RESUME: return "count_nt2_probe_kernel+count_nt2_resume_kernel";
    case CountSchedule::READS_SINGLE: return "count_nt2_reads_kernel";
    case CountSchedule::READS_LISTS: return "count_nt2_reads_probe_kernel+count_nt2_reads_kernel";
    case CountSchedule::READS_LANES: return "count_nt2_reads_probe_kernel+lcx_quad_reads_kernel+count_nt2_reads_pool_kernel";
    case CountSchedule::WIDE_SINGLE: return "count_nt2_wide_kernel";
    case CountSchedule::WIDE_TWO_PHASE: return "count_nt2_wide_probe_kernel+count_nt2_wide_kernel";
  }
  return "";
}

}  // namespace awry
