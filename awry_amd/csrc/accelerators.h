// accelerators.h -- seed tables and rungs, dense SA, N block, verify text, left-context index, position seeds, make_replica
// A part of awry_hip.hip (one translation unit): included there, in order, and not on its own.
#pragma once

namespace {

int default_seed_k(const HostIndex& h) {
  if (!narrow(h)) {  // wide rows: nucleotide only, 16-byte entries (+ 4 B scratch per entry while building)
    if (h.alphabet != NUCLEOTIDE) return 0;
    if (const char* e = getenv("AWRY_SEED_K")) return std::max(0, std::min(17, atoi(e)));
    int k = std::min(17, (int)std::floor(std::log((double)h.bwt_len) / std::log(4.0)) + 2);
    size_t free_b = 0;
    if (hbm_budget(&free_b))
      while (k > 1 && 20.0 * std::pow(4.0, k) > 0.7 * (double)free_b) k--;
    return std::max(1, k);
  }
  const bool nt = h.alphabet == NUCLEOTIDE;
  if (const char* e = getenv("AWRY_SEED_K")) return std::max(0, std::min(nt ? 17 : 7, atoi(e)));
  if (!nt) {  // amino: 20^k ~ 1..20 x bwt_len (Swiss-Prot 9e7 -> k = 7, 10 GB), same memory rule as below
    int k = (int)std::floor(std::log((double)h.bwt_len) / std::log(20.0)) + 1;
    k = std::max(1, std::min(k, 7));
    size_t free_b = 0;
    if (hbm_budget(&free_b))
      while (k > 1 && 8.5 * std::pow((double)AA_SEED_SIGMA, k) > 0.7 * (double)free_b) k--;
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
  while (k < 17 && (double)(1ull << (2 * k)) < 12.0 * (double)h.bwt_len) k++;
  size_t free_b = 0;
  if (hbm_budget(&free_b))
    while (k > 1 && (double)(10ull << (2 * k)) > 0.7 * (double)free_b) k--;  // 8 B + 2 B scratch per entry
  return k;
}

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

// The table for nucleotide k-mers of L < seed_k letters, built on first use and kept.  nullptr: not available (it does not
// fit the HBM budget, or AWRY_SEED_RUNGS=0) -- the caller falls back to LF steps from the last letter.  Which launches ask
// for one is the count plan's rule (count_plan.h, plan_kmers); the guard here keeps the table's size bounded whoever asks.
const SeedEntry* seed_rung(Replica& r, int L) {
  static const bool off = getenv("AWRY_SEED_RUNGS") && !strcmp(getenv("AWRY_SEED_RUNGS"), "0");
  if (off || r.wide || r.dev.alphabet != NUCLEOTIDE || L < SEED_RUNG_MIN || L > SEED_RUNG_MAX) return nullptr;
  std::lock_guard<std::mutex> lock(r.rung_mu);
  auto it = r.rungs.find(L);
  if (it != r.rungs.end()) return it->second.p;
  if (r.rungs_refused.count(L)) return nullptr;
  // 8 B per entry + a quarter of that while building must fit half of what is free now (AWRY_HBM_BUDGET_GB caps that figure),
  // and all rungs of a replica together stay below AWRY_SEED_RUNG_GB (default 48: every length 6..16 at once would be 46 GB)
  static const double rung_cap = [] { const char* e = getenv("AWRY_SEED_RUNG_GB"); return (e && atof(e) > 0 ? atof(e) : 48.0) * 1e9; }();
  double held = 0;
  for (const auto& kv : r.rungs) held += 8.0 * (double)kv.second.n;
  size_t free_b = 0;
  if (!hbm_budget(&free_b) || (double)(10ull << (2 * L)) > 0.5 * (double)free_b || held + (double)(8ull << (2 * L)) > rung_cap) {
    r.rungs_refused.insert(L);
    return nullptr;
  }
  int cur_dev = 0;
  HIP_CHECK(hipGetDevice(&cur_dev));
  if (cur_dev != r.device) HIP_CHECK(hipSetDevice(r.device));
  struct Restore { int dev, mine; ~Restore() { if (dev != mine) (void)hipSetDevice(dev); } } restore{cur_dev, r.device};  // the caller's device
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
// awry_debug_set_kmer_table_lines: the number of lines of tables built afterwards (rounded down to a power of two), whatever
// their load; 0 (the default): the policy below.  For tests: a table far too small overflows in most lines, and an L-mer whose
// tag does not fit beside so few line bits marks its line the same way -- both are searched as without the table.
std::atomic<uint64_t> g_kt_debug_lines{0};

void drop_kmer_table(Replica& r) {
  std::unique_lock<std::shared_mutex> lock(r.kt_mu);
  r.kt.tab.reset();  // (hipFree waits for the kernels that are queued)
  r.kt = Replica::KmerTable{};
  r.kt_refused.clear();
}

// Builds the table for length L in place of the one that is there; the caller holds r.kt_mu exclusively.  Like a rung
// (seed_rung): on the replica's own stream, synchronous, the table within half of the HBM that is free now (the only build
// scratch is one counter line), a refused length is remembered, an allocation that fails means "not available".
void build_kmer_table(Replica& r, int L) {
  r.kt.tab.reset();
  r.kt = Replica::KmerTable{};
  if (r.wide || !r.dev.lcx_key || !r.dev.lcx_rowpos || !r.dev.text4 || !r.dense_sa.p || r.dense_ratio != 1 || !r.seed.p || L <= r.seed_k || L > 32) return;
  int cur_dev = 0;
  HIP_CHECK(hipGetDevice(&cur_dev));
  if (cur_dev != r.device) HIP_CHECK(hipSetDevice(r.device));
  struct Restore { int dev, mine; ~Restore() { if (dev != mine) (void)hipSetDevice(dev); } } restore{cur_dev, r.device};  // the caller's device
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
    // lines: at most 8 keys per line on average (then a line of 16 slots overflows once in ~250), a power of two, and so many
    // that the tag -- the 2L - bits upper bits of the mixed key -- fits its field: for small texts that is the size
    uint32_t bits = 0;
    while ((8ull << bits) < h[2]) bits++;
    while (2 * L - (int)bits > KT_TAG_BITS) bits++;
    if (const uint64_t forced = g_kt_debug_lines.load()) {
      bits = 0;
      while ((2ull << bits) <= forced && bits < 40) bits++;
    }
    const uint64_t bytes = 128ull << bits;
    size_t free_b = 0;
    if (!hbm_budget(&free_b) || (double)bytes + 4096.0 > 0.5 * (double)free_b) { r.kt_refused.insert(L); return; }
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
  static const bool verbose = getenv("AWRY_VERBOSE") != nullptr;
  if (verbose) fprintf(stderr, "[awry replica %d] k-mer count table for L = %d: %llu entries in %llu lines (%llu overflowed), %.2f GB, built in %.1f ms\n", r.device, L,
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

void drop_lcx(Replica& r) {
  drop_kmer_table(r);  // it is made of the index's keys and the seed table's flags
  r.lcx_key.reset(); r.lcx_rowpos.reset(); r.lcx_inner.reset();
  r.dev.lcx_key = r.dev.lcx_rowpos = r.dev.lcx_inner = nullptr;
  for (auto& o : r.dev.lcx_off) o = 0;
}

void build_seed(awry_index* ix, Replica& r, int k) {
  drop_lcx(r);  // its flags live in the table's entries
  r.seed.reset();
  r.seed_k = 0;
  r.dev.seed = nullptr;
  r.dev.seed_k = 0;
  r.dev.seed_pos = 0;
  r.dev.ctx_extra = 0;
  r.seed64.reset();
  r.dev.seed64 = nullptr;
  if (k <= 0) return;
  if (r.wide) {  // 64-bit rows: 16-byte entries, nucleotide only
    require(ix->host.alphabet == NUCLEOTIDE, "a wide-row seed table needs a nucleotide index");
    require(k <= 17, "seed k-mer length must be <= 17");
    DevBuf<SeedEntry64> a;
    build_seed_table(r, true, k, a);
    r.seed64 = std::move(a);
    r.seed_k = k;
    r.dev.seed64 = r.seed64.p;
    r.dev.seed_k = k;
    return;
  }
  require(narrow(ix->host), "seed table needs an index with bwt_len < 2^32");
  const bool nt = ix->host.alphabet == NUCLEOTIDE;
  require(k <= (nt ? 17 : 7), "seed k-mer length must be <= 17 (nucleotide) / 7 (amino)");
  DevBuf<SeedEntry> a;
  build_seed_table(r, nt, k, a);
  r.seed = std::move(a);
  r.seed_k = k;
  r.dev.seed = r.seed.p;
  r.dev.seed_k = k;
}

// dense device SA for locate: ratio 0 = off (walk to the file's samples), r >= 1 = keep SA[j r] for every j as u32
void build_dense_sa(awry_index* ix, Replica& r, int ratio) {
  drop_kmer_table(r);  // (built from the ratio-1 dense SA and the text)
  r.text4.reset();  // the verify shortcut rides on the ratio-1 dense SA; it is re-enabled by build_verify()
  r.text8.reset();
  r.dev.text4 = nullptr;
  r.dev.text8 = nullptr;
  r.dense_sa.reset();
  r.dense_ratio = 0;
  r.dev.dense_sa = nullptr;
  r.dev.dense_ratio = 0;
  if (ratio <= 0) return;
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
  r.dev.dense_sa = r.dense_sa.p;
  r.dev.dense_ratio = r.dense_ratio;
}

// While locate has to walk (no ratio-1 dense SA), a nucleotide replica keeps the SA values of the BWT's N block: a walk
// that runs into an N run stops there instead of following the run (see DevIndex::sa_nblock).  4 B per N of the text.
void refresh_nblock(awry_index* ix, Replica& r) {
  const HostIndex& h = ix->host;
  const uint64_t lo = h.alphabet == NUCLEOTIDE ? h.prefix_sums[4] : 0, hi = h.alphabet == NUCLEOTIDE ? h.prefix_sums[5] : 0;
  const bool want = h.alphabet == NUCLEOTIDE && !r.wide && narrow(h) && r.dense_ratio != 1 && hi - lo >= 64;
  if (!want) {
    r.sa_nblock.reset();
    r.dev.sa_nblock = nullptr;
    return;
  }
  if (r.sa_nblock.p) return;  // depends on the index only
  DevBuf<uint32_t> d(hi - lo);
  const uint64_t nsamples = (h.bwt_len + h.sa_ratio - 1) / h.sa_ratio;
  hipLaunchKernelGGL(nblock_sa_kernel<NUCLEOTIDE>, dim3(grid_for(r, nsamples, 256, 64)), dim3(256), 0, r.stream, r.dev, nsamples,
                     (uint32_t)lo, (uint32_t)hi, d.p);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipStreamSynchronize(r.stream));
  r.sa_nblock = std::move(d);
  r.dev.sa_nblock = r.sa_nblock.p;
}

// seed-and-verify: needs the ratio-1 dense SA and the text, both recovered from the index on the device -- as 4-bit
// codes for the packed nucleotide kernels (text4) and as one symbol index per byte for the generic kernel (text8, any
// alphabet).  after_steps < 0 switches it off.
void build_verify(awry_index* ix, Replica& r, int after_steps) {
  drop_kmer_table(r);
  r.text4.reset();
  r.text8.reset();
  r.dev.text4 = nullptr;
  r.dev.text8 = nullptr;
  r.dev.verify_after = 0;
  if (after_steps < 0) return;
  require(!r.wide && narrow(ix->host), "seed-and-verify needs an index with bwt_len < 2^32");
  if (r.dense_ratio != 1) build_dense_sa(ix, r, 1);
  if (r.dense_ratio != 1 || !r.dense_sa.p) throw HipError("seed-and-verify: the ratio-1 dense SA is missing");
  const bool nt = ix->host.alphabet == NUCLEOTIDE;
  const dim3 g(grid_for(r, ix->host.bwt_len, 256)), b(256);
  DevBuf<uint8_t> t8(ix->host.bwt_len + 16);
  with_alphabet(ix->host.alphabet, [&](auto A) { hipLaunchKernelGGL(text8_scatter_kernel<A()>, g, b, 0, r.stream, r.dev, t8.p); });
  HIP_CHECK(hipGetLastError());
  if (nt) {
    const uint64_t nwords = (ix->host.bwt_len + 7) / 8 + 8;  // + slack: a 32-symbol window read touches 5 words
    DevBuf<uint32_t> t(nwords);
    HIP_CHECK(hipMemsetAsync(t.p, 0, nwords * 4, r.stream));
    hipLaunchKernelGGL(text4_scatter_kernel<NUCLEOTIDE>, g, b, 0, r.stream, r.dev, t.p);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(r.stream));
    r.text4 = std::move(t);
    r.dev.text4 = r.text4.p;
  }
  HIP_CHECK(hipStreamSynchronize(r.stream));
  r.text8 = std::move(t8);
  r.dev.text8 = r.text8.p;
  r.dev.verify_after = (uint32_t)after_steps;
}

bool lcx_wanted(const awry_index* ix) {
  static const bool off = getenv("AWRY_LCX") && !strcmp(getenv("AWRY_LCX"), "0");
  return !off && ix->lcx_request != 0;
}

// The left-context index of a nucleotide replica (layout.h, lcx.hip.h): 16 B per row for the keys and the (position, row)
// pairs, 0.6 B for the sampled levels.  Built from what is resident anyway -- the final seed table (its 2+ row entries name
// the buckets), the ratio-1 dense SA, the 4-bit text -- in chunks of rows cut at bucket boundaries: per chunk two stable radix
// sorts (context key, then bucket) order the covered rows, which then go back to their buckets' own row slots.
// Skipped (returns false) when the HBM that is free does not hold it and its build scratch with room to spare.
bool build_lcx(awry_index* ix, Replica& r) {
  drop_lcx(r);
  const HostIndex& h = ix->host;
  if (r.wide || h.alphabet != NUCLEOTIDE || !r.seed.p || r.seed_k < 8 || !r.dev.text4 || !r.dense_sa.p || r.dense_ratio != 1) return false;
  const uint64_t N = h.bwt_len, nfinal = 1ull << (2 * r.seed_k);
  uint64_t lev_n[8] = {0}, lev_off[8] = {0}, inner_total = 16;
  for (int t = 1; t <= 7; t++) {
    lev_n[t] = ((((N - 1) >> (4 * t)) + 1 + 15) / 16) * 16 + 16;  // whole nodes, one to spare
    lev_off[t] = inner_total;
    inner_total += lev_n[t];
  }
  const double resident = 16.0 * (double)(N + 32) + 8.0 * (double)inner_total;
  size_t free_b = 0;
  if (!hbm_budget(&free_b)) return false;
  constexpr double PER_ROW = 96.0;  // build scratch per row of a chunk (row info 17 B, covered rows 4 B, two double-buffered pair sorts 48 B, rocPRIM's own)
  if (resident + PER_ROW * (double)(1u << 24) > 0.75 * (double)free_b) return false;
  const uint64_t chunk = (uint64_t)std::max(1.0 * (1u << 24), std::min(1.0 * (1u << 28), (0.75 * (double)free_b - resident) / PER_ROW));
  const uint32_t max_bucket = (uint32_t)std::min<uint64_t>(1u << 24, chunk / 2);
  static const bool verbose = getenv("AWRY_VERBOSE") != nullptr;
  const auto t_begin = std::chrono::steady_clock::now();
  DevBuf<uint64_t> key(N + 32), rowpos(N + 32), inner(inner_total);
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
    hipLaunchKernelGGL(lcx_sample_kernel, dim3(grid_for(r, lev_n[t], 256)), dim3(256), 0, s, key.p, N, t, inner.p + lev_off[t], lev_n[t]);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipStreamSynchronize(s));
  r.lcx_key = std::move(key);
  r.lcx_rowpos = std::move(rowpos);
  r.lcx_inner = std::move(inner);
  r.dev.lcx_key = r.lcx_key.p;
  r.dev.lcx_rowpos = r.lcx_rowpos.p;
  r.dev.lcx_inner = r.lcx_inner.p;
  for (int t = 0; t < 8; t++) r.dev.lcx_off[t] = (uint32_t)lev_off[t];
  if (verbose) fprintf(stderr, "[awry replica %d] left-context index built in %.2f s (%.1f GB)\n", r.device,
                       std::chrono::duration<double>(std::chrono::steady_clock::now() - t_begin).count(), resident / 1e9);
  return true;
}

// Position seeds are kept exactly while they pay: nucleotide replica with the verify accelerators resident and a table
// sparse enough for the two-phase schedules (the kernels of those schedules settle a singleton from the text and never
// need its row; the other schedules and the generic kernel would have to start such queries over without the table).
// Called after anything that changes the table or the accelerators.  AWRY_SEED_POS=0 keeps rows.
// awry_debug_set_ctx_extra_cap: an upper bound on the extra context letters of tables converted afterwards; -1 (the
// default): none.  For tests: the E = 0 and E = 2 of GRCh38- and chr1-scale indexes at a text of a few thousand letters.
std::atomic<int> g_ctx_extra_cap{-1};

void sync_seed_mode(awry_index* ix, Replica& r) {
  const HostIndex& h = ix->host;
  static const bool off = getenv("AWRY_SEED_POS") && !strcmp(getenv("AWRY_SEED_POS"), "0");
  if (r.wide) return;  // wide rows: no position seeds (32-bit structures)
  const bool nt = h.alphabet == NUCLEOTIDE;
  // nucleotide: text4 resident and the two-phase schedules are the policy; amino: text8 resident (its only consumer, the
  // generic kernel, then finishes singletons against the text)
  const bool want = !off && narrow(h) && r.seed_k > 0 && r.seed.p && r.dense_ratio == 1 && r.dense_sa.p &&
                    (nt ? (r.dev.text4 && (1ull << (2 * r.seed_k)) / 3 >= h.bwt_len) : r.dev.text8 != nullptr);
  const bool want_lcx = want && nt && lcx_wanted(ix);
  if (want == (r.dev.seed_pos != 0)) {
    if (want && want_lcx != (r.dev.lcx_key != nullptr)) {
      if (want_lcx) build_lcx(ix, r);
      else { build_seed(ix, r, r.seed_k); sync_seed_mode(ix, r); }  // (the table carries the index's flags: a fresh one, then position seeds again)
    }
    return;
  }
  if (!want) {  // rows again: rebuild (the row of a position is not recoverable without an inverse SA)
    build_seed(ix, r, r.seed_k);
    return;
  }
  uint64_t nfinal = 1;
  for (int j = 0; j < r.seed_k; j++) nfinal *= nt ? 4 : AA_SEED_SIGMA;
  // context letters beyond the 14 of the count field ride in the top bits of sp that positions of this text never use
  int extra = nt ? (int)std::min<uint64_t>(15, (32 - std::min<uint64_t>(32, h.sa_bits)) / 2) : 0;
  if (const int cap = g_ctx_extra_cap.load(); cap >= 0) extra = std::min(extra, cap);
  hipLaunchKernelGGL(seed_rows_to_positions_kernel, dim3(grid_for(r, nfinal, 256)), dim3(256), 0, r.stream, r.seed.p, nfinal, r.dense_sa.p,
                     nt ? SEED_CNT_SAT : AA_SEED_CNT_SAT, nt ? r.dev.text4 : nullptr, extra, nt ? nullptr : r.dev.text8);
  r.dev.ctx_extra = (uint32_t)extra;
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipStreamSynchronize(r.stream));
  r.dev.seed_pos = 1;
  if (want_lcx) build_lcx(ix, r);
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
  static const bool verbose = getenv("AWRY_VERBOSE") != nullptr;
  auto t_last = std::chrono::steady_clock::now();
  auto lap = [&](const char* what) {  // AWRY_VERBOSE: where the seconds of a replica's construction go
    if (!verbose) return;
    const auto t = std::chrono::steady_clock::now();
    fprintf(stderr, "[awry replica %d] %s: %.2f s\n", device, what, std::chrono::duration<double>(t - t_last).count());
    t_last = t;
  };
  r->blocks.alloc(h.blocks.size());
  r->sa_words.alloc(h.sa_words.size() + 1);  // +1: the straddle read of the last sample never leaves the buffer
  r->seq_starts.alloc(std::max<size_t>(1, h.seq_starts.size()));
  HIP_CHECK(hipMemcpy(r->blocks.p, h.blocks.data(), h.blocks.size() * 8, hipMemcpyHostToDevice));
  HIP_CHECK(hipMemset(r->sa_words.p, 0, (h.sa_words.size() + 1) * 8));
  if (!h.sa_words.empty()) HIP_CHECK(hipMemcpy(r->sa_words.p, h.sa_words.data(), h.sa_words.size() * 8, hipMemcpyHostToDevice));
  if (!h.seq_starts.empty())
    HIP_CHECK(hipMemcpy(r->seq_starts.p, h.seq_starts.data(), h.seq_starts.size() * 8, hipMemcpyHostToDevice));
  r->wide = !narrow(h);
  DevIndex& d = r->dev;
  d.seed64 = nullptr;
  d.blocks = r->blocks.p;
  d.sa_words = r->sa_words.p;
  d.seed = nullptr;
  d.seq_starts = r->seq_starts.p;
  d.seq_bucket = nullptr;
  d.seq_bucket_shift = d.seq_bucket_pad = 0;
  if (h.seq_starts.size() > (size_t)LOC_SEQ_LDS && h.seq_starts.size() < (1ull << 32)) {
    // about four buckets per record (at most 2^22): a position's record is then one of the one or two its bucket touches
    const uint64_t nseq = h.seq_starts.size();
    uint64_t want = 1;
    while (want < 4 * nseq && want < (1ull << 22)) want <<= 1;
    uint32_t shift = 0;
    while ((((h.bwt_len - 1) >> shift) + 1) > want) shift++;
    const uint64_t nb = ((h.bwt_len - 1) >> shift) + 1;
    std::vector<uint32_t> tab(nb + 1);
    uint64_t rec = 0;
    for (uint64_t b = 0; b < nb; b++) {
      const uint64_t p0 = b << shift;
      while (rec + 1 < nseq && h.seq_starts[rec + 1] <= p0) rec++;
      tab[b] = (uint32_t)rec;
    }
    tab[nb] = (uint32_t)(nseq - 1);
    r->seq_bucket.alloc(nb + 1);
    HIP_CHECK(hipMemcpy(r->seq_bucket.p, tab.data(), (nb + 1) * 4, hipMemcpyHostToDevice));
    d.seq_bucket = r->seq_bucket.p;
    d.seq_bucket_shift = shift;
  }
  d.nblocks = h.nblocks;
  d.bwt_len = h.bwt_len;
  d.sentinel_row = h.sentinel_row;
  d.nseq = h.seq_starts.size();
  for (int i = 0; i < 24; i++) d.prefix_sums[i] = i < (int)h.prefix_sums.size() ? h.prefix_sums[i] : 0;
  d.sa_bits = (uint32_t)h.sa_bits;
  d.sa_ratio = (uint32_t)h.sa_ratio;
  d.alphabet = h.alphabet;
  d.seed_k = 0;
  d.dense_sa = nullptr;
  d.text4 = nullptr;
  d.text8 = nullptr;
  d.dense_ratio = 0;
  d.verify_after = 0;
  d.sa_nblock = nullptr;
  d.seed_pos = 0;
  d.ctx_extra = 0;
  lap("index upload");
  build_seed(ix, *r, ix->seed_k_request < 0 ? default_seed_k(h) : ix->seed_k_request);
  lap("seed table");
  build_dense_sa(ix, *r, ix->dense_ratio_request);
  lap("dense SA");
  int vreq = ix->verify_request;
  if (vreq == -2) {  // policy: keep the accelerators (dense SA 4 B + text 1.5 B / 1 B per symbol) resident when they fit comfortably
    vreq = -1;
    const char* e = getenv("AWRY_VERIFY");
    size_t free_b = 0;
    if (!(e && !strcmp(e, "0")) && !r->wide && narrow(h) && hbm_budget(&free_b) && (double)h.bwt_len * 7.0 < 0.5 * (double)free_b)
      vreq = e && atoi(e) > 0 ? atoi(e) : 2;
  }
  if (vreq >= 0) build_verify(ix, *r, vreq);
  lap("verify accelerators (dense SA at ratio 1, text)");
  r->verify_kmers = ix->verify_kmers_request;
  r->kt_mode = ix->kmer_table_request;
  refresh_nblock(ix, *r);
  sync_seed_mode(ix, *r);
  lap("block-of-sample table, seed mode");
  return r;
}

}  // namespace
