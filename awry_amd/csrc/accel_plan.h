// accel_plan.h -- which device-only accelerators a replica holds and how large, as pure functions of the index's facts, what the
// replica holds now and the HBM that is free
// Plain C++ (no HIP): accelerators.h fills the facts, reads the free-HBM figure at the moment each decision is due and builds what
// these functions say; tests/test_accel_plan_cpu.py compiles the header on its own.  DESIGN.md, "The accelerator plan".
#pragma once
#include <stdint.h>

#include <algorithm>
#include <cmath>

#include "layout.h"  // NUCLEOTIDE, AA_SEED_SIGMA, KT_TAG_BITS

namespace awry {

// HBM the policies may plan with: what is free on the device at the moment of the decision, capped by AWRY_HBM_BUDGET_GB
// (replica.h hbm_free).  known == false: the runtime could not say -- nothing that needs room is admitted, the seed k is not cut.
struct HbmFree {
  bool known = false;
  uint64_t bytes = 0;
};

// What the policies read of the index, of the requests of awry_index and of the environment (accelerators.h accel_facts).
struct AccelFacts {
  int alphabet = NUCLEOTIDE;
  uint64_t bwt_len = 0;
  uint64_t sa_bits = 0;      // bits of a position of this text (HostIndex::sa_bits)
  bool wide = false;         // 64-bit rows: none of the 32-bit accelerators
  uint64_t nblock_rows = 0;  // rows whose suffix starts with N (nucleotide; else 0)
  int seed_k_request = -1;   // awry_set_seed_kmer_len: -1 the policy
  int verify_request = -2;   // awry_set_verify: -2 the policy, -1 off, >= 0 LF steps before the text comparison
  int lcx_request = -1;      // awry_set_lcx: 0 no left-context index
  // the environment, as values
  bool seed_k_env = false;  // AWRY_SEED_K is set ...
  int seed_k_env_value = 0;  // ... to this number
  bool verify_env_off = false;  // AWRY_VERIFY=0
  int verify_env_steps = 0;     // AWRY_VERIFY as a number (0: not set, or no number)
  bool seed_pos_off = false;    // AWRY_SEED_POS=0
  bool lcx_env_off = false;     // AWRY_LCX=0
  int ctx_extra_cap = -1;       // awry_debug_set_ctx_extra_cap: -1 none
};

// What the replica holds now (accelerators.h accel_held).
struct AccelHeld {
  int seed_k = 0;
  bool seed = false;         // the seed table of 8-byte entries is resident
  bool seed_pos = false;     // its singletons hold text positions
  uint32_t dense_ratio = 0;  // the dense SA: 0 none
  bool text4 = false, text8 = false;
  bool lcx = false;  // the left-context index
};

// ---- the seed table's k ----
// The policy for an index of bwt_len rows; AWRY_SEED_K overrides it within the lengths the tables are built for.
inline int default_seed_k(const AccelFacts& f, HbmFree free) {
  if (f.wide) {  // wide rows: nucleotide only, 16-byte entries (+ 4 B scratch per entry while building)
    if (f.alphabet != NUCLEOTIDE) return 0;
    if (f.seed_k_env) return std::max(0, std::min(17, f.seed_k_env_value));
    int k = std::min(17, (int)std::floor(std::log((double)f.bwt_len) / std::log(4.0)) + 2);
    if (free.known)
      while (k > 1 && 20.0 * std::pow(4.0, k) > 0.7 * (double)free.bytes) k--;
    return std::max(1, k);
  }
  const bool nt = f.alphabet == NUCLEOTIDE;
  if (f.seed_k_env) return std::max(0, std::min(nt ? 17 : 7, f.seed_k_env_value));
  if (!nt) {  // amino: 20^k ~ 1..20 x bwt_len (Swiss-Prot 9e7 -> k = 7, 10 GB), same memory rule as below
    int k = (int)std::floor(std::log((double)f.bwt_len) / std::log(20.0)) + 1;
    k = std::max(1, std::min(k, 7));
    if (free.known)
      while (k > 1 && 8.5 * std::pow((double)AA_SEED_SIGMA, k) > 0.7 * (double)free.bytes) k--;
    return k;
  }
  // A dozen table entries per suffix or more: the smallest k with 4^k >= 12 x bwt_len, at most 17 (GRCh38: 17, 137 GB of the
  // 288 GB HBM and 5.5 entries per suffix -- 18 would not fit; chr1: 16, 34 GB; E. coli: 13).  A random k-mer's entry is
  // then empty or a singleton whose BWT symbol rarely matches, so a query costs one probe plus ~0.1 steps instead of ~16
  // steps (27 block reads), and a k-mer from the text rarely shares its seed with another one.  (Round 1 took
  // floor(log4 bwt_len) + 2, i.e. 4..16 entries per suffix; chr1 sat at the low end of that with k = 15: k = 16 counts
  // random 31-mers 8 %, 31-mers from the text 36 % and 101-bp reads 18 % faster.)  The table and its build scratch (1/4 of
  // it) must fit in 70 % of the free HBM, else k drops.
  int k = 1;
  while (k < 17 && (double)(1ull << (2 * k)) < 12.0 * (double)f.bwt_len) k++;
  if (free.known)
    while (k > 1 && (double)(10ull << (2 * k)) > 0.7 * (double)free.bytes) k--;  // 8 B + 2 B scratch per entry
  return k;
}
// the k the replica's table is built with: the request, or the policy (free: read before the table is built)
inline int seed_k_wanted(const AccelFacts& f, HbmFree free) { return f.seed_k_request < 0 ? default_seed_k(f, free) : f.seed_k_request; }

// ---- seed-and-verify ----
// The steps a new replica's verify accelerators are built with, -1: none.  The policy keeps them (dense SA 4 B + text 1.5 B /
// 1 B per symbol) resident when they fit comfortably: 7 B per symbol under half of what is free once the seed table and the
// requested dense SA are there.  AWRY_VERIFY=0 switches the policy off, AWRY_VERIFY=<steps> sets its step count (default 2).
inline int verify_steps_wanted(const AccelFacts& f, HbmFree free) {
  if (f.verify_request != -2) return f.verify_request;
  if (f.verify_env_off || f.wide || !free.known || !((double)f.bwt_len * 7.0 < 0.5 * (double)free.bytes)) return -1;
  return f.verify_env_steps > 0 ? f.verify_env_steps : 2;
}

// ---- the SA of the N block ----
// While locate has to walk (no ratio-1 dense SA), a nucleotide replica keeps the SA values of the BWT's N block: a walk that
// runs into an N run stops there instead of following the run (see DevIndex::sa_nblock).  4 B per N of the text.
inline bool nblock_wanted(const AccelFacts& f, const AccelHeld& h) {
  return f.alphabet == NUCLEOTIDE && !f.wide && h.dense_ratio != 1 && f.nblock_rows >= 64;
}

// ---- position seeds ----
// Kept exactly while they pay: the verify accelerators resident -- nucleotide: text4, and a table sparse enough for the
// two-phase schedules to be the policy (count_plan.h; their kernels settle a singleton from the text and never need its row,
// the other schedules and the generic kernel would have to start such queries over without the table); amino: text8 (its only
// consumer, the generic kernel, then finishes singletons against the text).  AWRY_SEED_POS=0 keeps rows.
inline bool seed_pos_wanted(const AccelFacts& f, const AccelHeld& h) {
  if (f.seed_pos_off || f.wide || h.seed_k <= 0 || !h.seed || h.dense_ratio != 1) return false;
  return f.alphabet == NUCLEOTIDE ? h.text4 && (1ull << (2 * h.seed_k)) / 3 >= f.bwt_len : h.text8;
}
// E: context letters beyond the 14 of the count field ride in the top bits of sp that positions of this text never use
inline int ctx_extra(const AccelFacts& f) {
  const int extra = f.alphabet == NUCLEOTIDE ? (int)std::min<uint64_t>(15, (32 - std::min<uint64_t>(32, f.sa_bits)) / 2) : 0;
  return f.ctx_extra_cap >= 0 ? std::min(extra, f.ctx_extra_cap) : extra;
}

// ---- the left-context index ----
inline bool lcx_wanted(const AccelFacts& f) { return !f.lcx_env_off && f.lcx_request != 0; }
// it is built from the final seed table in positions (its 2+ row entries name the buckets), the ratio-1 dense SA and the 4-bit text
inline bool lcx_possible(const AccelFacts& f, const AccelHeld& h) {
  return !f.wide && f.alphabet == NUCLEOTIDE && h.seed && h.seed_k >= 8 && h.text4 && h.dense_ratio == 1;
}
// Sizes: 16 B per row for the keys and the (position, row) pairs, 8 B per entry of the sampled levels 1..7 (level t: every
// 16^t-th key in whole nodes of 16, one node to spare, at lev_off[t] of lcx_inner; its first 16 words are unused).  Built in
// chunks of rows; admitted when what stays resident and the build scratch of the smallest chunk (2^24 rows) fit in 0.75 of what
// is free at build time; the chunk then takes what is left of that, up to 2^28 rows, and buckets of more than max_bucket rows
// stay out of the index.
struct LcxPlan {
  uint64_t lev_n[8] = {0}, lev_off[8] = {0}, inner_total = 16;
  double resident = 0;
  bool admitted = false;
  uint64_t chunk = 0;
  uint32_t max_bucket = 0;
};
inline LcxPlan lcx_plan(uint64_t bwt_len, HbmFree free) {
  LcxPlan p;
  for (int t = 1; t <= 7; t++) {
    p.lev_n[t] = ((((bwt_len - 1) >> (4 * t)) + 1 + 15) / 16) * 16 + 16;  // whole nodes, one to spare
    p.lev_off[t] = p.inner_total;
    p.inner_total += p.lev_n[t];
  }
  p.resident = 16.0 * (double)(bwt_len + 32) + 8.0 * (double)p.inner_total;
  constexpr double PER_ROW = 96.0;  // build scratch per row of a chunk (row info 17 B, covered rows 4 B, two double-buffered pair sorts 48 B, rocPRIM's own)
  if (!free.known || p.resident + PER_ROW * (double)(1u << 24) > 0.75 * (double)free.bytes) return p;
  p.admitted = true;
  p.chunk = (uint64_t)std::max(1.0 * (1u << 24), std::min(1.0 * (1u << 28), (0.75 * (double)free.bytes - p.resident) / PER_ROW));
  p.max_bucket = (uint32_t)std::min<uint64_t>(1u << 24, p.chunk / 2);
  return p;
}

// ---- the rungs (count_plan.h SEED_RUNG_MIN .. SEED_RUNG_MAX: which launches ask for one is the count plan's rule) ----
inline bool rung_possible(bool rungs_off, bool wide, int alphabet, int L) {
  return !rungs_off && !wide && alphabet == NUCLEOTIDE && L >= 6 && L <= 16;
}
// 8 B per entry + a quarter of that while building must fit half of what is free at build time, and all rungs of a replica
// together (held_bytes: those there) stay below AWRY_SEED_RUNG_GB (cap_env_gb; not set or <= 0: 48 -- every length 6..16 at
// once would be 46 GB)
inline bool rung_admitted(int L, double held_bytes, double cap_env_gb, HbmFree free) {
  const double cap = (cap_env_gb > 0 ? cap_env_gb : 48.0) * 1e9;
  return free.known && !((double)(10ull << (2 * L)) > 0.5 * (double)free.bytes) && !(held_bytes + (double)(8ull << (2 * L)) > cap);
}

// ---- the k-mer count table (layout.h KT_*) ----
// made of the left-context index's keys and the seed table's flags, for lengths beyond the seed table's k
inline bool kmer_table_possible(const AccelHeld& h, bool wide, int L) {
  return !wide && h.lcx && h.text4 && h.dense_ratio == 1 && h.seed && L > h.seed_k && L <= 32;
}
// 2^bits lines for `keys` distinct L-mers: at most 8 keys per line on average (then a line of 16 slots overflows once in ~250),
// and so many that the tag -- the 2L - bits upper bits of the mixed key -- fits its field: for small texts that is the size.
// forced_lines (awry_debug_set_kmer_table_lines; 0: none): that many lines, rounded down to a power of two, whatever the load.
inline uint32_t kmer_table_bits(uint64_t keys, int L, uint64_t forced_lines) {
  uint32_t bits = 0;
  while ((8ull << bits) < keys) bits++;
  while (2 * L - (int)bits > KT_TAG_BITS) bits++;
  if (forced_lines) {
    bits = 0;
    while ((2ull << bits) <= forced_lines && bits < 40) bits++;
  }
  return bits;
}
// the table (128 B per line; the only build scratch is one counter line) within half of what is free at build time
inline bool kmer_table_admitted(uint32_t bits, HbmFree free) {
  return free.known && !((double)(128ull << bits) + 4096.0 > 0.5 * (double)free.bytes);
}

// ---- the record buckets of locate (DevIndex::seq_bucket) ----
// For indexes of more records than the locate kernels keep in LDS (lds_records): about four buckets of 2^shift positions per
// record (at most 2^22) -- a position's record is then one of the one or two its bucket touches.
struct SeqBucketPlan {
  bool wanted = false;
  uint32_t shift = 0;
  uint64_t buckets = 0;
};
inline SeqBucketPlan seq_bucket_plan(uint64_t bwt_len, uint64_t nseq, uint64_t lds_records) {
  SeqBucketPlan p;
  if (!(nseq > lds_records && nseq < (1ull << 32))) return p;
  p.wanted = true;
  uint64_t want = 1;
  while (want < 4 * nseq && want < (1ull << 22)) want <<= 1;
  while ((((bwt_len - 1) >> p.shift) + 1) > want) p.shift++;
  p.buckets = ((bwt_len - 1) >> p.shift) + 1;
  return p;
}

}  // namespace awry
