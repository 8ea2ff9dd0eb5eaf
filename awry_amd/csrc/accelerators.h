// accelerators.h -- seed tables and rungs, dense SA, N block, verify text, left-context index, position seeds, make_replica
// A part of awry_hip.hip (one translation unit): included there, in order, and not on its own.
// What a replica holds and how large is decided in accel_plan.h (pure functions); this file fills their inputs, builds and drops.
// A builder builds ONE accelerator into its DevBuf and the replica's host-side state and ends with publish(); what a change
// takes with it is drop()'s table; settle() brings the rest in line.  DESIGN.md, "The accelerator plan".
#pragma once

namespace {

// ---- the inputs of the plan ----
// awry_debug_set_ctx_extra_cap: an upper bound on the extra context letters of tables converted afterwards; -1 (the
// default): none.  For tests: the E = 0 and E = 2 of GRCh38- and chr1-scale indexes at a text of a few thousand letters.
std::atomic<int> g_ctx_extra_cap{-1};
// awry_debug_set_kmer_table_lines: the number of lines of tables built afterwards (rounded down to a power of two), whatever
// their load; 0 (the default): the policy.  For tests: a table far too small overflows in most lines, and an L-mer whose
// tag does not fit beside so few line bits marks its line the same way -- both are searched as without the table.
std::atomic<uint64_t> g_kt_debug_lines{0};

// The switches of the environment that are read once per process: all of them at the first call, which is the first
// make_replica.  (Each used to be read at the first use of its own function -- AWRY_SEED_RUNGS at the first seed_rung, say --
// so a process that sets one between its first replica and that first use no longer changes it; nothing in the project does.)
struct AccelEnv {
  bool seed_pos_off, lcx_off, rungs_off, verbose;
  double rung_gb;
};
const AccelEnv& accel_env() {
  static const AccelEnv env = [] {
    auto zero = [](const char* name) { const char* e = getenv(name); return e && !strcmp(e, "0"); };
    const char* gb = getenv("AWRY_SEED_RUNG_GB");
    return AccelEnv{zero("AWRY_SEED_POS"), zero("AWRY_LCX"), zero("AWRY_SEED_RUNGS"), getenv("AWRY_VERBOSE") != nullptr, gb ? atof(gb) : 0.0};
  }();
  return env;
}

// (AWRY_SEED_K and AWRY_VERIFY are read per call, by the two callers that decide with them)
AccelFacts accel_facts(const awry_index* ix, bool wide) {
  const HostIndex& h = ix->host;
  AccelFacts f;
  f.alphabet = h.alphabet;
  f.bwt_len = h.bwt_len;
  f.sa_bits = h.sa_bits;
  f.wide = wide;
  f.nblock_rows = h.alphabet == NUCLEOTIDE ? h.prefix_sums[5] - h.prefix_sums[4] : 0;
  f.seed_k_request = ix->seed_k_request;
  f.verify_request = ix->verify_request;
  f.lcx_request = ix->lcx_request;
  f.seed_pos_off = accel_env().seed_pos_off;
  f.lcx_env_off = accel_env().lcx_off;
  f.ctx_extra_cap = g_ctx_extra_cap.load();
  return f;
}

AccelHeld accel_held(const Replica& r) {
  AccelHeld h;
  h.seed_k = r.seed_k;
  h.seed = r.seed.p != nullptr;
  h.seed_pos = r.seed_pos;
  h.dense_ratio = r.dense_sa.p ? r.dense_ratio : 0;
  h.text4 = r.text4.p != nullptr;
  h.text8 = r.text8.p != nullptr;
  h.lcx = r.lcx_key.p && r.lcx_rowpos.p;
  return h;
}

// The seed k of the index's request: the policy looks at the rows of replicas built NOW (narrow() reads
// awry_debug_force_wide_rows), also when awry_set_seed_kmer_len asks for a replica built before the switch changed.
int wanted_seed_k(const awry_index* ix) {
  AccelFacts f = accel_facts(ix, !narrow(ix->host));
  if (f.seed_k_request >= 0) return f.seed_k_request;
  if (const char* e = getenv("AWRY_SEED_K")) {
    f.seed_k_env = true;
    f.seed_k_env_value = atoi(e);
  }
  return seed_k_wanted(f, hbm_free());
}

// The verify steps a new replica is built with: the request, or the policy from AWRY_VERIFY and what is free at this moment.
int wanted_verify_steps(const awry_index* ix, const Replica& r) {
  AccelFacts f = accel_facts(ix, r.wide || !narrow(ix->host));
  if (f.verify_request != -2) return f.verify_request;
  if (const char* e = getenv("AWRY_VERIFY")) {
    f.verify_env_off = !strcmp(e, "0");
    f.verify_env_steps = atoi(e);
  }
  return verify_steps_wanted(f, hbm_free());
}

// ---- what the kernels see ----
// Every accelerator field of r.dev, from the owning buffers and the host-side state.  drop() ends with it, and a builder calls it
// right after it has moved its buffers in, behind its last statement that can throw: a builder that throws has changed nothing
// since the publish of the drop before it, so r.dev describes what is held whichever way control leaves.  (Once per builder and
// not once per settle: the next builder's kernels take r.dev and read what this one built.)
void publish(Replica& r) {
  r.dev.seed = r.seed.p;
  r.dev.seed64 = r.seed64.p;
  r.dev.seed_k = r.seed_k;
  r.dev.seed_pos = r.seed_pos ? 1 : 0;
  r.dev.ctx_extra = (uint32_t)r.ctx_extra;
  r.dev.dense_sa = r.dense_sa.p;
  r.dev.dense_ratio = r.dense_ratio;
  r.dev.text4 = r.text4.p;
  r.dev.text8 = r.text8.p;
  r.dev.verify_after = r.verify_after;
  r.dev.sa_nblock = r.sa_nblock.p;
  r.dev.lcx_key = r.lcx_key.p;
  r.dev.lcx_rowpos = r.lcx_rowpos.p;
  r.dev.lcx_inner = r.lcx_inner.p;
  for (int t = 0; t < 8; t++) r.dev.lcx_off[t] = r.lcx_off[t];
}

// the replica's device for the rest of the scope, then the caller's again
struct OnDevice {
  int prev = 0, mine;
  explicit OnDevice(int device) : mine(device) {
    HIP_CHECK(hipGetDevice(&prev));
    if (prev != mine) HIP_CHECK(hipSetDevice(mine));
  }
  ~OnDevice() { if (prev != mine) (void)hipSetDevice(prev); }
};

void drop_kmer_table(Replica& r) {
  std::unique_lock<std::shared_mutex> lock(r.kt_mu);
  r.kt.tab.reset();  // (hipFree waits for the kernels that are queued)
  r.kt = Replica::KmerTable{};
  r.kt_refused.clear();
}

// ---- what depends on what ----
// Dropping (or rebuilding) an accelerator drops what was made from it:
//   seed table          -> left-context index (its flags live in the table's entries)
//   left-context index  -> count table (it is made of the index's keys and the seed table's flags)
//   dense SA            -> texts (the verify shortcut rides on the ratio-1 dense SA), count table
//   texts               -> count table
// Position seeds and the left-context index also need the texts and the ratio-1 dense SA to be RESIDENT; that is settle()'s rule,
// not a drop: they outlive a rebuild of the same texts.  The N block follows the dense ratio (settle); the rungs depend on the
// index alone and survive everything.
enum Accel : unsigned { SEED = 1, DENSE_SA = 2, TEXTS = 4, LCX = 8, KMER_TABLE = 16, NBLOCK = 32 };
void drop(Replica& r, unsigned what) {
  if (what & SEED) what |= LCX;
  if (what & DENSE_SA) what |= TEXTS;
  if (what & (LCX | TEXTS)) what |= KMER_TABLE;
  if (what & KMER_TABLE) drop_kmer_table(r);
  if (what & LCX) {
    r.lcx_key.reset(); r.lcx_rowpos.reset(); r.lcx_inner.reset();
    for (auto& o : r.lcx_off) o = 0;
  }
  if (what & SEED) {
    r.seed.reset();
    r.seed64.reset();
    r.seed_k = 0;
    r.seed_pos = false;
    r.ctx_extra = 0;
  }
  if (what & TEXTS) {
    r.text4.reset();
    r.text8.reset();
  }
  if (what & DENSE_SA) {
    r.dense_sa.reset();
    r.dense_ratio = 0;
  }
  if (what & NBLOCK) r.sa_nblock.reset();
  publish(r);
}

// ---- the seed table ----
// the complete sigma^k table of (first row, count + BWT symbol of a singleton) entries -- SeedEntry for a 32-bit-row replica,
// SeedEntry64 (nucleotide only) for a wide-row one -- built level by level on the replica's own stream (see seed_extend_kernel);
// synchronous
template <class Entry>
void build_seed_table(Replica& r, bool nt, int k, DevBuf<Entry>& out) {
  constexpr bool wide = std::is_same<Entry, SeedEntry64>::value;
  const uint64_t sigma = nt ? 4 : AA_SEED_SIGMA;
  uint64_t nfinal = 1;
  for (int j = 0; j < k; j++) nfinal *= sigma;
  DevBuf<Entry> a(nfinal), b(std::max<uint64_t>(sigma, nfinal / sigma));
  // level j lands in `a` when (k - j) is even, so the last level is in `a`
  Entry* cur = ((k - 1) % 2 == 0) ? a.p : b.p;
  if (nt) hipLaunchKernelGGL(seed_level1_kernel<Entry>, dim3(1), dim3(256), 0, r.stream, r.dev, cur);
  else if constexpr (!wide) hipLaunchKernelGGL(aa_seed_level1_kernel, dim3(1), dim3(256), 0, r.stream, r.dev, cur);
  uint64_t nchild = sigma;
  for (int j = 2; j <= k; j++) {
    Entry* nxt = ((k - j) % 2 == 0) ? a.p : b.p;
    nchild *= sigma;
    if (nt) hipLaunchKernelGGL(seed_extend_kernel<Entry>, dim3(grid_for(r, nchild * 4, 256)), dim3(256), 0, r.stream, r.dev, cur, nxt, nchild);
    else if constexpr (!wide) hipLaunchKernelGGL(aa_seed_extend_kernel, dim3(grid_for(r, nchild, 256)), dim3(256), 0, r.stream, r.dev, cur, nxt, nchild);
    cur = nxt;
  }
  if constexpr (wide) hipLaunchKernelGGL(seed64_finalize_kernel, dim3(grid_for(r, nfinal, 256)), dim3(256), 0, r.stream, r.dev, a.p, nfinal);
  else if (nt) hipLaunchKernelGGL(seed_finalize_kernel, dim3(grid_for(r, nfinal, 256)), dim3(256), 0, r.stream, r.dev, a.p, nfinal);
  else hipLaunchKernelGGL(aa_seed_finalize_kernel, dim3(grid_for(r, nfinal, 256)), dim3(256), 0, r.stream, r.dev, a.p, nfinal);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipStreamSynchronize(r.stream));
  out = std::move(a);
}

// the replica's table in rows, k >= 1; none is resident
void build_seed(awry_index* ix, Replica& r, int k) {
  if (r.wide) {  // 64-bit rows: 16-byte entries, nucleotide only
    require(ix->host.alphabet == NUCLEOTIDE, "a wide-row seed table needs a nucleotide index");
    require(k <= 17, "seed k-mer length must be <= 17");
    build_seed_table(r, true, k, r.seed64);
  } else {
    require(narrow(ix->host), "seed table needs an index with bwt_len < 2^32");
    const bool nt = ix->host.alphabet == NUCLEOTIDE;
    require(k <= (nt ? 17 : 7), "seed k-mer length must be <= 17 (nucleotide) / 7 (amino)");
    build_seed_table(r, nt, k, r.seed);
  }
  r.seed_k = k;
  publish(r);
}

// singletons of the row table become text positions with 14 + extra letters of left context (seed_rows_to_positions_kernel)
void seed_to_positions(Replica& r, bool nt, int extra) {
  uint64_t nfinal = 1;
  for (int j = 0; j < r.seed_k; j++) nfinal *= nt ? 4 : AA_SEED_SIGMA;
  hipLaunchKernelGGL(seed_rows_to_positions_kernel, dim3(grid_for(r, nfinal, 256)), dim3(256), 0, r.stream, r.seed.p, nfinal, r.dense_sa.p,
                     nt ? SEED_CNT_SAT : AA_SEED_CNT_SAT, nt ? r.text4.p : nullptr, extra, nt ? nullptr : r.text8.p);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipStreamSynchronize(r.stream));
  r.ctx_extra = extra;
  r.seed_pos = true;
  publish(r);
}

// The table for nucleotide k-mers of L < seed_k letters, built on first use and kept.  nullptr: not available (it does not
// fit the HBM budget, or AWRY_SEED_RUNGS=0) -- the caller falls back to LF steps from the last letter.  Which launches ask
// for one is the count plan's rule (count_plan.h, plan_kmers); the guard here keeps the table's size bounded whoever asks.
static_assert(SEED_RUNG_MIN == 6 && SEED_RUNG_MAX == 16, "rung_possible (accel_plan.h) admits the lengths the count plan asks for");
const SeedEntry* seed_rung(Replica& r, int L) {
  if (!rung_possible(accel_env().rungs_off, r.wide, r.dev.alphabet, L)) return nullptr;
  std::lock_guard<std::mutex> lock(r.rung_mu);
  auto it = r.rungs.find(L);
  if (it != r.rungs.end()) return it->second.p;
  if (r.rungs_refused.count(L)) return nullptr;
  double held = 0;
  for (const auto& kv : r.rungs) held += 8.0 * (double)kv.second.n;
  if (!rung_admitted(L, held, accel_env().rung_gb, hbm_free())) {
    r.rungs_refused.insert(L);
    return nullptr;
  }
  OnDevice on(r.device);
  DevBuf<SeedEntry> t;
  try {
    build_seed_table(r, true, L, t);
  } catch (const HipError&) {  // (hipMalloc: the budget was an estimate)
    (void)hipGetLastError();
    r.rungs_refused.insert(L);
    return nullptr;
  }
  const SeedEntry* p = t.p;
  r.rungs.emplace(L, std::move(t));
  return p;
}

// ---- the k-mer count table (layout.h KT_*, kmer_table.hip.h) ----
// Builds the table for length L in place of the one that is there; the caller holds r.kt_mu exclusively.  Like a rung
// (seed_rung): on the replica's own stream, synchronous, admitted against the HBM that is free now, a refused length is
// remembered, an allocation that fails means "not available".
void build_kmer_table(Replica& r, int L) {
  r.kt.tab.reset();
  r.kt = Replica::KmerTable{};
  if (!kmer_table_possible(accel_held(r), r.wide, L)) return;
  OnDevice on(r.device);
  const auto t_begin = std::chrono::steady_clock::now();
  try {
    DevBuf<unsigned long long> stats(4);
    unsigned long long h[4] = {0, 0, 0, 0};
    HIP_CHECK(hipMemsetAsync(stats.p, 0, 32, r.stream));
    const dim3 g(grid_for(r, r.dev.bwt_len, 256)), b(256);
    hipLaunchKernelGGL(kt_scan_kernel<false>, g, b, 0, r.stream, r.dev, L, (uint64_t*)nullptr, 0u, stats.p);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(h, stats.p, 32, hipMemcpyDeviceToHost, r.stream));
    HIP_CHECK(hipStreamSynchronize(r.stream));
    const uint32_t bits = kmer_table_bits(h[2], L, g_kt_debug_lines.load());  // h[2]: the distinct keys
    const uint64_t bytes = 128ull << bits;
    if (!kmer_table_admitted(bits, hbm_free())) { r.kt_refused.insert(L); return; }
    DevBuf<uint64_t> tab(16ull << bits);
    HIP_CHECK(hipMemsetAsync(tab.p, 0, bytes, r.stream));
    hipLaunchKernelGGL(kt_scan_kernel<true>, g, b, 0, r.stream, r.dev, L, tab.p, bits, stats.p);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(h, stats.p, 32, hipMemcpyDeviceToHost, r.stream));
    HIP_CHECK(hipStreamSynchronize(r.stream));
    r.kt.tab = std::move(tab);
    r.kt.L = L;
    r.kt.bits = bits;
    r.kt.entries = h[0];
    r.kt.overflowed = h[1];
  } catch (const HipError&) {  // (hipMalloc: the budget was an estimate)
    (void)hipGetLastError();
    r.kt.tab.reset();
    r.kt = Replica::KmerTable{};
    r.kt_refused.insert(L);
    return;
  }
  r.kt.build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
  if (accel_env().verbose) fprintf(stderr, "[awry replica %d] k-mer count table for L = %d: %llu entries in %llu lines (%llu overflowed), %.2f GB, built in %.1f ms\n", r.device, L,
                                   (unsigned long long)r.kt.entries, 1ull << r.kt.bits, (unsigned long long)r.kt.overflowed, (double)(128ull << r.kt.bits) / 1e9, r.kt.build_ms);
}

// The table of length L for a launch: nullptr when it is not resident and is not to be built (or cannot be).  On success
// `lock` is held (shared): the caller keeps it until the kernel that takes the pointer is queued.
const Replica::KmerTable* kmer_table(Replica& r, int L, bool build, std::shared_lock<std::shared_mutex>& lock) {
  lock = std::shared_lock<std::shared_mutex>(r.kt_mu);
  if (r.kt.L == L && r.kt.tab.p) return &r.kt;
  const bool refused = r.kt_refused.count(L) != 0;
  lock.unlock();
  if (!build || refused) return nullptr;
  {
    std::unique_lock<std::shared_mutex> excl(r.kt_mu);
    if (!(r.kt.L == L && r.kt.tab.p) && !r.kt_refused.count(L)) build_kmer_table(r, L);
  }
  lock.lock();
  if (r.kt.L == L && r.kt.tab.p) return &r.kt;
  lock.unlock();
  return nullptr;
}

// ---- dense SA, N block, texts ----
// dense device SA for locate: SA[j ratio] for every j as u32, ratio >= 1; none is resident
void build_dense_sa(awry_index* ix, Replica& r, int ratio) {
  require(!r.wide && ix->host.bwt_len < (1ull << 32), "a dense device SA needs an index with 32-bit rows (bwt_len < 2^32)");
  const uint64_t nentries = (ix->host.bwt_len + ratio - 1) / ratio;
  const uint64_t nsamples = (ix->host.bwt_len + ix->host.sa_ratio - 1) / ix->host.sa_ratio;  // one chain per file sample
  DevBuf<uint32_t> d(nentries);
  const dim3 g(grid_for(r, nsamples, 256, 64)), b(256);
  with_alphabet(r.dev.alphabet, [&](auto A) { hipLaunchKernelGGL(densify_sa_kernel<A()>, g, b, 0, r.stream, r.dev, (uint32_t)ratio, nsamples, d.p); });
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipStreamSynchronize(r.stream));
  r.dense_sa = std::move(d);
  r.dense_ratio = (uint32_t)ratio;
  publish(r);
}

// the SA values of the BWT's N block (accel_plan.h nblock_wanted); depends on the index only
void build_nblock(awry_index* ix, Replica& r) {
  const HostIndex& h = ix->host;
  const uint64_t lo = h.prefix_sums[4], hi = h.prefix_sums[5];
  DevBuf<uint32_t> d(hi - lo);
  const uint64_t nsamples = (h.bwt_len + h.sa_ratio - 1) / h.sa_ratio;
  hipLaunchKernelGGL(nblock_sa_kernel<NUCLEOTIDE>, dim3(grid_for(r, nsamples, 256, 64)), dim3(256), 0, r.stream, r.dev, nsamples,
                     (uint32_t)lo, (uint32_t)hi, d.p);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipStreamSynchronize(r.stream));
  r.sa_nblock = std::move(d);
  publish(r);
}

// the text for seed-and-verify, recovered from the index and the ratio-1 dense SA on the device -- as 4-bit codes for the packed
// nucleotide kernels (text4) and as one symbol index per byte for the generic kernel (text8, any alphabet); none is resident
void build_texts(awry_index* ix, Replica& r, int after_steps) {
  if (r.dense_ratio != 1 || !r.dense_sa.p) throw HipError("seed-and-verify: the ratio-1 dense SA is missing");
  const bool nt = ix->host.alphabet == NUCLEOTIDE;
  const dim3 g(grid_for(r, ix->host.bwt_len, 256)), b(256);
  DevBuf<uint8_t> t8(ix->host.bwt_len + 16);
  with_alphabet(ix->host.alphabet, [&](auto A) { hipLaunchKernelGGL(text8_scatter_kernel<A()>, g, b, 0, r.stream, r.dev, t8.p); });
  HIP_CHECK(hipGetLastError());
  DevBuf<uint32_t> t4;
  if (nt) {
    const uint64_t nwords = (ix->host.bwt_len + 7) / 8 + 8;  // + slack: a 32-symbol window read touches 5 words
    t4.alloc(nwords);
    HIP_CHECK(hipMemsetAsync(t4.p, 0, nwords * 4, r.stream));
    hipLaunchKernelGGL(text4_scatter_kernel<NUCLEOTIDE>, g, b, 0, r.stream, r.dev, t4.p);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(r.stream));
  }
  HIP_CHECK(hipStreamSynchronize(r.stream));
  r.text4 = std::move(t4);
  r.text8 = std::move(t8);
  r.verify_after = (uint32_t)after_steps;
  publish(r);
}

// ---- the left-context index ----
// The left-context index of a nucleotide replica (layout.h, lcx.hip.h), sized by `plan` (accel_plan.h lcx_plan; admitted).
// Built from what is resident anyway -- the final seed table (its 2+ row entries name the buckets), the ratio-1 dense SA, the
// 4-bit text -- in chunks of rows cut at bucket boundaries: per chunk two stable radix sorts (context key, then bucket) order the
// covered rows, which then go back to their buckets' own row slots.  None is resident.
void build_lcx(awry_index* ix, Replica& r, const LcxPlan& plan) {
  const uint64_t N = ix->host.bwt_len, nfinal = 1ull << (2 * r.seed_k), chunk = plan.chunk;
  const uint32_t max_bucket = plan.max_bucket;
  const bool verbose = accel_env().verbose;
  const auto t_begin = std::chrono::steady_clock::now();
  DevBuf<uint64_t> key(N + 32), rowpos(N + 32), inner(plan.inner_total);
  hipStream_t s = r.stream;
  HIP_CHECK(hipMemsetAsync(key.p, 0, (N + 32) * 8, s));
  HIP_CHECK(hipMemsetAsync(rowpos.p, 0, (N + 32) * 8, s));
  hipLaunchKernelGGL(lcx_flag_big_kernel, dim3(grid_for(r, nfinal, 256)), dim3(256), 0, s, r.seed.p, nfinal, max_bucket);
  HIP_CHECK(hipGetLastError());
  {
    const uint64_t cap = std::min(chunk + max_bucket, N);
    DevBuf<uint64_t> bkey(cap), ckey(cap), k1a(cap), k1b(cap), b1a(cap), b1b(cap);
    DevBuf<uint8_t> valid(cap);
    DevBuf<uint32_t> slot(cap + 1), p1a(cap), p1b(cap), q2a(cap), q2b(cap), small(4);
    size_t tmp_bytes = 0, need = 0;
    {  // rocPRIM scratch: the largest of the three calls at full capacity
      rocprim::double_buffer<uint64_t> dk(k1a.p, k1b.p);
      rocprim::double_buffer<uint32_t> dv(p1a.p, p1b.p);
      HIP_CHECK(rocprim::radix_sort_pairs(nullptr, need, dk, dv, (size_t)cap, 0, 64, s));
      tmp_bytes = need;
      HIP_CHECK(rocprim::select(nullptr, need, rocprim::counting_iterator<uint32_t>(0), valid.p, slot.p, small.p, (size_t)cap, s));
      tmp_bytes = std::max(tmp_bytes, need);
    }
    DevBuf<uint8_t> tmp(tmp_bytes + 256);
    uint32_t h_small[4];
    uint64_t r0 = 0, covered = 0, nchunks = 0;
    while (r0 < N) {
      uint64_t r1 = std::min(N, r0 + chunk);
      if (r1 < N) {  // cut at the first row of the bucket that holds row r1
        hipLaunchKernelGGL(lcx_bucket_start_kernel, dim3(1), dim3(64), 0, s, r.dev, (uint32_t)r1, max_bucket, small.p + 1);
        HIP_CHECK(hipMemcpyAsync(h_small, small.p + 1, 4, hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        if (h_small[0] > r0 && h_small[0] <= r1) r1 = h_small[0];
      }
      const uint64_t n = r1 - r0;
      const dim3 g(grid_for(r, n, 256)), b(256);
      hipLaunchKernelGGL(lcx_rowinfo_kernel, g, b, 0, s, r.dev, (uint32_t)r0, (uint32_t)n, max_bucket, bkey.p, ckey.p, valid.p);
      need = tmp_bytes;
      HIP_CHECK(rocprim::select(tmp.p, need, rocprim::counting_iterator<uint32_t>(0), valid.p, slot.p, small.p, (size_t)n, s));
      HIP_CHECK(hipMemcpyAsync(h_small, small.p, 4, hipMemcpyDeviceToHost, s));
      HIP_CHECK(hipStreamSynchronize(s));
      const uint64_t nv = h_small[0];
      if (nv) {
        const dim3 gv(grid_for(r, nv, 256));
        hipLaunchKernelGGL(lcx_gather_u64_kernel, gv, b, 0, s, ckey.p, slot.p, nv, k1a.p);
        hipLaunchKernelGGL(lcx_iota_kernel, gv, b, 0, s, p1a.p, nv);
        rocprim::double_buffer<uint64_t> dk(k1a.p, k1b.p);
        rocprim::double_buffer<uint32_t> dv(p1a.p, p1b.p);
        need = tmp_bytes;
        HIP_CHECK(rocprim::radix_sort_pairs(tmp.p, need, dk, dv, (size_t)nv, 0, 64, s));
        // bucket keys in the order of the first sort, then the (stable) sort by bucket
        hipLaunchKernelGGL(lcx_gather2_u64_kernel, gv, b, 0, s, bkey.p, dv.current(), slot.p, nv, b1a.p);
        hipLaunchKernelGGL(lcx_iota_kernel, gv, b, 0, s, q2a.p, nv);
        rocprim::double_buffer<uint64_t> db(b1a.p, b1b.p);
        rocprim::double_buffer<uint32_t> dq(q2a.p, q2b.p);
        need = tmp_bytes;
        HIP_CHECK(rocprim::radix_sort_pairs(tmp.p, need, db, dq, (size_t)nv, 0, 2 * r.seed_k + 1, s));
        hipLaunchKernelGGL(lcx_place_kernel, gv, b, 0, s, r.dev, (uint32_t)r0, nv, dk.current(), dv.current(), dq.current(), slot.p, key.p, rowpos.p);
        hipLaunchKernelGGL(lcx_tail_kernel, gv, b, 0, s, r.dev, (uint32_t)r0, nv, db.current(), slot.p, key.p, r.seed.p);
        HIP_CHECK(hipGetLastError());
      }
      covered += nv;
      nchunks++;
      r0 = r1;
    }
    HIP_CHECK(hipStreamSynchronize(s));
    if (verbose) fprintf(stderr, "[awry replica %d] left-context index: %llu of %llu rows in buckets of 2..%u rows, %llu chunks of <= %llu rows\n", r.device,
                         (unsigned long long)covered, (unsigned long long)N, max_bucket, (unsigned long long)nchunks, (unsigned long long)chunk);
  }
  for (int t = 1; t <= 7; t++)
    hipLaunchKernelGGL(lcx_sample_kernel, dim3(grid_for(r, plan.lev_n[t], 256)), dim3(256), 0, s, key.p, N, t, inner.p + plan.lev_off[t], plan.lev_n[t]);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipStreamSynchronize(s));
  r.lcx_key = std::move(key);
  r.lcx_rowpos = std::move(rowpos);
  r.lcx_inner = std::move(inner);
  for (int t = 0; t < 8; t++) r.lcx_off[t] = (uint32_t)plan.lev_off[t];
  publish(r);
  if (verbose) fprintf(stderr, "[awry replica %d] left-context index built in %.2f s (%.1f GB)\n", r.device,
                       std::chrono::duration<double>(std::chrono::steady_clock::now() - t_begin).count(), plan.resident / 1e9);
}

// ---- one accelerator changes ... ----
// Each drops the accelerator with what was made from it (drop) and builds it anew as asked -- also when what is asked for is
// what is there.  settle() follows.
void rebuild_seed(awry_index* ix, Replica& r, int k) {
  drop(r, SEED);
  if (k > 0) build_seed(ix, r, k);
}

// ratio 0 = off (locate walks to the file's samples)
void rebuild_dense_sa(awry_index* ix, Replica& r, int ratio) {
  drop(r, DENSE_SA);
  if (ratio > 0) build_dense_sa(ix, r, ratio);
}

// seed-and-verify after `after_steps` LF steps; < 0 switches it off (and leaves the dense SA as it is)
void rebuild_verify(awry_index* ix, Replica& r, int after_steps) {
  r.verify_after = 0;
  drop(r, TEXTS);
  if (after_steps < 0) return;
  require(!r.wide && narrow(ix->host), "seed-and-verify needs an index with bwt_len < 2^32");
  if (r.dense_ratio != 1) rebuild_dense_sa(ix, r, 1);
  build_texts(ix, r, after_steps);
}

// ---- ... and the rest follows ----
// What an entry point calls after it has changed one accelerator (and after nothing else, awry_set_lcx): the N block, the
// seed table in rows or positions and the left-context index as accel_plan.h wants them for what is resident now.
void settle(awry_index* ix, Replica& r) {
  const AccelFacts f = accel_facts(ix, r.wide || !narrow(ix->host));
  const bool nt = f.alphabet == NUCLEOTIDE;
  // the N block follows the dense ratio
  if (!nblock_wanted(f, accel_held(r))) {
    if (r.sa_nblock.p) drop(r, NBLOCK);
  } else if (!r.sa_nblock.p) build_nblock(ix, r);
  // a fresh table in rows where positions are no longer wanted (the row of a position is not recoverable without an inverse
  // SA), or carry the flags of a left-context index that is no longer wanted
  const bool pos = seed_pos_wanted(f, accel_held(r));
  const bool lcx = pos && nt && lcx_wanted(f);
  if (r.seed_pos && (!pos || (r.lcx_key.p && !lcx))) rebuild_seed(ix, r, r.seed_k);
  if (pos && !r.seed_pos) seed_to_positions(r, nt, ctx_extra(f));
  // the index, when the HBM that is free now holds it and its build scratch with room to spare (else the next settle tries again)
  if (lcx && !r.lcx_key.p && lcx_possible(f, accel_held(r))) {
    const LcxPlan plan = lcx_plan(f.bwt_len, hbm_free());
    if (plan.admitted) build_lcx(ix, r, plan);
  }
}

// The knobs: `change` on every replica, then settle.  (awry_set_seed_kmer_len did not refresh the N block before there was one
// settle: the block depends on the index and the dense ratio alone, and every path that changes the ratio -- make_replica,
// awry_set_locate_sa_ratio, awry_set_verify -- settles, so the step finds nothing to do there.  The one exception: a knob call that
// threw between changing the ratio and its settle -- awry_set_verify whose texts did not fit, after it had built the ratio-1 dense
// SA -- leaves the block as it was, and the next settle, also that of awry_set_seed_kmer_len, then brings it in line.)
template <class Change>
void change_replicas(awry_index* ix, Change&& change) {
  for (size_t s = 0; s < ix->reps.size(); s++) {
    Replica& r = replica(ix, (int)s);
    change(r);
    settle(ix, r);
  }
}

// ---- a new replica ----
// the index itself: blocks, sampled SA, record starts and their buckets, and the index fields of r.dev
void upload_index(const HostIndex& h, Replica& r) {
  r.blocks.alloc(h.blocks.size());
  r.sa_words.alloc(h.sa_words.size() + 1);  // +1: the straddle read of the last sample never leaves the buffer
  r.seq_starts.alloc(std::max<size_t>(1, h.seq_starts.size()));
  HIP_CHECK(hipMemcpy(r.blocks.p, h.blocks.data(), h.blocks.size() * 8, hipMemcpyHostToDevice));
  HIP_CHECK(hipMemset(r.sa_words.p, 0, (h.sa_words.size() + 1) * 8));
  if (!h.sa_words.empty()) HIP_CHECK(hipMemcpy(r.sa_words.p, h.sa_words.data(), h.sa_words.size() * 8, hipMemcpyHostToDevice));
  if (!h.seq_starts.empty())
    HIP_CHECK(hipMemcpy(r.seq_starts.p, h.seq_starts.data(), h.seq_starts.size() * 8, hipMemcpyHostToDevice));
  DevIndex& d = r.dev;
  d.blocks = r.blocks.p;
  d.sa_words = r.sa_words.p;
  d.seq_starts = r.seq_starts.p;
  if (const SeqBucketPlan sb = seq_bucket_plan(h.bwt_len, h.seq_starts.size(), LOC_SEQ_LDS); sb.wanted) {
    const uint64_t nseq = h.seq_starts.size(), nb = sb.buckets;
    std::vector<uint32_t> tab(nb + 1);
    uint64_t rec = 0;
    for (uint64_t b = 0; b < nb; b++) {
      const uint64_t p0 = b << sb.shift;
      while (rec + 1 < nseq && h.seq_starts[rec + 1] <= p0) rec++;
      tab[b] = (uint32_t)rec;
    }
    tab[nb] = (uint32_t)(nseq - 1);
    r.seq_bucket.alloc(nb + 1);
    HIP_CHECK(hipMemcpy(r.seq_bucket.p, tab.data(), (nb + 1) * 4, hipMemcpyHostToDevice));
    d.seq_bucket = r.seq_bucket.p;
    d.seq_bucket_shift = sb.shift;
  }
  d.nblocks = h.nblocks;
  d.bwt_len = h.bwt_len;
  d.sentinel_row = h.sentinel_row;
  d.nseq = h.seq_starts.size();
  for (int i = 0; i < 24; i++) d.prefix_sums[i] = i < (int)h.prefix_sums.size() ? h.prefix_sums[i] : 0;
  d.sa_bits = (uint32_t)h.sa_bits;
  d.sa_ratio = (uint32_t)h.sa_ratio;
  d.alphabet = h.alphabet;
}

std::unique_ptr<Replica> make_replica(awry_index* ix, int device) {
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev == 0) throw NoDeviceError("no HIP device available (there is no CPU search path)");
  require(device >= 0 && device < ndev, "device id out of range");
  HIP_CHECK(hipSetDevice(device));
  // replicas of one GPU are built one after the other (each sizes its seed table and accelerators from the HBM that is
  // free when its turn comes); replicas of different GPUs build concurrently
  static std::mutex build_mu[64];
  std::lock_guard<std::mutex> build_lock(build_mu[device & 63]);
  auto r = std::make_unique<Replica>();
  r->device = device;
  hipDeviceProp_t prop;
  HIP_CHECK(hipGetDeviceProperties(&prop, device));
  r->num_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  {
    const void* fused[4] = {(const void*)count_nt2_probe_resume_kernel<false, false>, (const void*)count_nt2_probe_resume_kernel<false, true>,
                            (const void*)count_nt2_probe_resume_kernel<true, false>, (const void*)count_nt2_probe_resume_kernel<true, true>};
    for (int i = 0; i < 4; i++) {
      int per_cu = 0;
      HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fused[i], 256, 0));
      r->probe_resume_per_cu[i] = std::max(1, std::min(per_cu, 8));
    }
    const void* lcx_reads[2] = {(const void*)lcx_quad_reads_kernel<false>, (const void*)lcx_quad_reads_kernel<true>};
    for (int i = 0; i < 2; i++) {
      int per_cu = 0;
      HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, lcx_reads[i], 256, 0));
      r->lcx_reads_grid[i] = (unsigned)r->num_cus * (unsigned)std::max(1, per_cu);
    }
  }
  HIP_CHECK(hipStreamCreateWithFlags(&r->stream, hipStreamNonBlocking));
  for (auto& ls : r->lane_stream) HIP_CHECK(hipStreamCreateWithFlags(&ls, hipStreamNonBlocking));
  HIP_CHECK(hipStreamCreateWithFlags(&r->copy_in, hipStreamNonBlocking));
  HIP_CHECK(hipStreamCreateWithFlags(&r->copy_out, hipStreamNonBlocking));
  HIP_CHECK(hipEventCreate(&r->ev0));
  HIP_CHECK(hipEventCreate(&r->ev1));
  const HostIndex& h = ix->host;
  auto t_last = std::chrono::steady_clock::now();
  auto lap = [&](const char* what) {  // AWRY_VERBOSE: where the seconds of a replica's construction go
    if (!accel_env().verbose) return;
    const auto t = std::chrono::steady_clock::now();
    fprintf(stderr, "[awry replica %d] %s: %.2f s\n", device, what, std::chrono::duration<double>(t - t_last).count());
    t_last = t;
  };
  r->wide = !narrow(h);
  upload_index(h, *r);
  lap("index upload");
  rebuild_seed(ix, *r, wanted_seed_k(ix));
  lap("seed table");
  rebuild_dense_sa(ix, *r, ix->dense_ratio_request);
  lap("dense SA");
  // (the verify policy looks at what is free once the seed table and the requested dense SA are there)
  if (const int steps = wanted_verify_steps(ix, *r); steps >= 0) rebuild_verify(ix, *r, steps);
  lap("verify accelerators (dense SA at ratio 1, text)");
  r->verify_kmers = ix->verify_kmers_request;
  r->kt_mode = ix->kmer_table_request;
  settle(ix, *r);
  lap("block-of-sample table, seed mode");
  return r;
}

}  // namespace
