// host_count.h -- chunking, the lane scaffold of the pipelined host paths, the count pipelines
// A part of awry_hip.hip (one translation unit): included there, in order, and not on its own.
#pragma once

namespace {

// ---- host batch drivers ----------------------------------------------------------------------------

struct Shard { uint64_t lo, hi; };

std::vector<Shard> shard_queries(uint64_t n, size_t parts) {  // query i -> replica floor(i * G / n): contiguous
  std::vector<Shard> out(parts);
  for (size_t g = 0; g < parts; g++) out[g] = Shard{n * g / parts, n * (g + 1) / parts};
  return out;
}

// cut [lo, hi) into chunks bounded in queries and bytes; copies: what the device holds per query given (2: both strands)
std::vector<Shard> chunk_queries(const uint64_t* qoff, uint64_t lo, uint64_t hi, uint64_t copies = 1) {
  const uint64_t MAXQ = (1ull << 24) / copies, MAXB = (1ull << 29) / copies;
  std::vector<Shard> out;
  uint64_t a = lo;
  while (a < hi) {
    uint64_t b = std::min(hi, a + MAXQ);
    while (b > a + 1 && qoff[b] - qoff[a] > MAXB) b = a + (b - a) / 2;
    out.push_back(Shard{a, b});
    a = b;
  }
  return out;
}

struct ChunkBuffers {
  DevBuf<uint8_t> q, status;
  DevBuf<uint64_t> off, counts, ranges;
  std::vector<uint64_t> h_off;
  std::vector<uint8_t> h_status;
};

// upload one chunk and run the generic count kernel; leaves counts / ranges / status on the device
void run_count_chunk(Replica& r, ChunkBuffers& cb, const uint8_t* qbytes, const uint64_t* qoff, Shard c, bool want_ranges,
                     bool allow_verify = true, int ref_kmer_len = -1) {
  const uint64_t n = c.hi - c.lo, base = qoff[c.lo], nbytes = qoff[c.hi] - base;
  cb.h_off.resize(n + 1);
  for (uint64_t i = 0; i <= n; i++) {
    if (qoff[c.lo + i] < base || (i && qoff[c.lo + i] < qoff[c.lo + i - 1])) throw ArgError("query offsets must be non-decreasing");
    cb.h_off[i] = qoff[c.lo + i] - base;
  }
  if (cb.q.n < nbytes + 16) cb.q.alloc(nbytes + 16);  // the kernel reads whole aligned 8-byte words
  if (cb.off.n < n + 1) cb.off.alloc(n + 1);
  if (cb.counts.n < n) cb.counts.alloc(n);
  if (cb.status.n < n) cb.status.alloc(n);
  if (want_ranges && cb.ranges.n < 2 * n) cb.ranges.alloc(2 * n);
  if (nbytes) HIP_CHECK(hipMemcpyAsync(cb.q.p, qbytes + base, nbytes, hipMemcpyHostToDevice, r.stream));
  HIP_CHECK(hipMemcpyAsync(cb.off.p, cb.h_off.data(), (n + 1) * 8, hipMemcpyHostToDevice, r.stream));
  launch_count_ascii(r, cb.q.p, cb.off.p, n, cb.counts.p, want_ranges ? cb.ranges.p : nullptr, cb.status.p, r.stream, allow_verify, 0, ref_kmer_len);
  cb.h_status.resize(n);
  HIP_CHECK(hipMemcpyAsync(cb.h_status.data(), cb.status.p, n, hipMemcpyDeviceToHost, r.stream));
}

[[noreturn]] void raise_bad_query(uint64_t query, uint8_t status) {
  static const char* why[] = {"", "empty query", "query contains '$' or '#'", "query contains a non-ASCII byte"};
  static const char* why_pattern[] = {"pattern contains a byte that is no class letter of the index's alphabet",
                                      "pattern has more than 16 class positions (AWRY_MAX_CLASS_POSITIONS)",
                                      "pattern search abandoned at the expansion cap (AWRY_PATTERN_MAX_EXPANSIONS)"};
  if (status >= Q_NOT_CLASS_LETTER && status <= Q_EXPANSION_CAP) throw QueryError("query " + std::to_string(query) + ": " + why_pattern[status - Q_NOT_CLASS_LETTER]);
  throw QueryError("query " + std::to_string(query) + ": " + why[status & 3] + " (undefined in the reference: src/fm_index.rs:406, src/bwt.rs:126-128)");
}
// raises INVALID_QUERY naming the first query of status[0, n) that the reference leaves undefined
void check_status(const uint8_t* status, size_t n, uint64_t first_query) {
  for (size_t i = 0; i < n; i++)
    if (status[i] != Q_OK) raise_bad_query(first_query + i, status[i]);
}
void check_status(const ChunkBuffers& cb, uint64_t first_query) { check_status(cb.h_status.data(), cb.h_status.size(), first_query); }
// the same from the one word the kernels keep per chunk: (index of its lowest rejected query << 8 | status), ~0 when there is none
void raise_first_bad(uint64_t word, uint64_t chunk_lo) {
  if (word != ~0ull) raise_bad_query(chunk_lo + (word >> 8), (uint8_t)(word & 0xFF));
}

// pins a caller-owned host range for the duration of a batch so that H2D/D2H run as real async DMA
struct HostPin {
  void* p = nullptr;
  HostPin(const void* ptr, size_t bytes) {
    if (ptr && bytes >= (8u << 20) && hipHostRegister(const_cast<void*>(ptr), bytes, hipHostRegisterDefault) == hipSuccess) p = const_cast<void*>(ptr);
    else (void)hipGetLastError();
  }
  ~HostPin() { if (p) (void)hipHostUnregister(p); }
};

// Can a shard of queries take the packed kernels, and how?  uniform: every query has Lmax letters; ragged: lengths in
// [1, Lmax], packed at a stride of W = ceil(Lmax / 32) words (accepted while that stride wastes little: the words of
// a query may take up to ~2x its own bytes).  Whether the letters are all ACGT is found out on the device.
struct PackedPlan {
  bool ok = false, ragged = false;
  uint64_t Lmax = 0;
};
PackedPlan plan_packed(const uint64_t* qoff, Shard sh) {
  PackedPlan plan;
  if (sh.hi <= sh.lo) return plan;
  const uint64_t n = sh.hi - sh.lo;
  auto scan = [&](uint64_t lo, uint64_t hi, uint64_t& mn, uint64_t& mx) {  // branch-free so the loop vectorises
    uint64_t a = ~0ull, b = 0;
    for (uint64_t i = lo; i < hi; i++) {
      const uint64_t d = qoff[i + 1] - qoff[i];
      a = d < a ? d : a;
      b = d > b ? d : b;
    }
    mn = a;
    mx = b;
  };
  uint64_t mn = ~0ull, mx = 0;
  if (n < (1u << 18)) {
    scan(sh.lo, sh.hi, mn, mx);
  } else {  // on the worker pool
    const uint64_t grain = 1u << 16, pieces = (n + grain - 1) / grain;
    std::vector<uint64_t> mns(pieces, ~0ull), mxs(pieces, 0);
    HostPool::instance().run(pieces, [&](uint64_t t) { scan(sh.lo + t * grain, std::min(sh.hi, sh.lo + (t + 1) * grain), mns[t], mxs[t]); });
    for (uint64_t t = 0; t < pieces; t++) { mn = std::min(mn, mns[t]); mx = std::max(mx, mxs[t]); }
  }
  if (mn == 0 || mx > 4096 || qoff[sh.hi] < qoff[sh.lo]) return plan;  // empty queries are the generic path's to reject
  plan.Lmax = mx;
  plan.ragged = mn != mx;
  if (plan.ragged) {
    const uint64_t bytes = qoff[sh.hi] - qoff[sh.lo], W = (mx + 31) / 32;
    if (mx > 512 || W * 8 * n > 2 * bytes + 16 * n) return plan;
  }
  plan.ok = true;
  return plan;
}

// chunks of a packed shard: at most max_q queries and ~max_bytes of ASCII each
std::vector<Shard> packed_chunks(const uint64_t* qoff, Shard sh, uint64_t max_q, uint64_t max_bytes) {
  std::vector<Shard> out;
  uint64_t a = sh.lo;
  while (a < sh.hi) {
    uint64_t b = std::min(sh.hi, a + max_q);
    if (qoff[b] - qoff[a] > max_bytes) {
      b = (uint64_t)(std::upper_bound(qoff + a, qoff + b + 1, qoff[a] + max_bytes) - qoff) - 1;
      b = std::max(b, a + 1);
    }
    out.push_back(Shard{a, b});
    a = b;
  }
  return out;
}

// ---- what the pipelined host paths share: lane preparation, the listed reads, counts out, retirement ----

void ensure_event(hipEvent_t& e) { if (!e) HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming)); }
template <class T>
void ensure(DevBuf<T>& b, size_t n) { if (b.n < n) b.alloc(n); }  // grow-only, like PinBuf::ensure

// every exit of a pipelined host call, normal or not, leaves the replica's lanes idle (declared after whatever pins caller
// memory, so that it runs before the unpinning)
struct DrainLanes {
  Replica& r;
  ~DrainLanes() {
    bool any = false;
    for (int li = 0; li < Replica::NLANES; li++)
      if (r.lanes[li].busy) { (void)hipStreamSynchronize(r.lane_stream[li]); r.lanes[li].busy = false; any = true; }
    for (int li = 0; li < 2; li++) {
      if (r.loc_lanes[li].stage) { (void)hipStreamSynchronize(r.lane_stream[li]); any = true; }
      r.loc_lanes[li].stage = 0;
    }
    if (any) { (void)hipStreamSynchronize(r.copy_in); (void)hipStreamSynchronize(r.copy_out); }
  }
};

// count lane li for chunks of up to cap_q queries: its stream and events, the counts on the device (64-bit, and narrowed) and
// their pinned 32-bit staging, the first-bad word and its pinned copy
PackedLane& prepare_count_lane(Replica& r, int li, uint64_t cap_q) {
  PackedLane& ln = r.lanes[li];
  ln.s = r.lane_stream[li];
  ensure_event(ln.done);
  ensure_event(ln.ev_in);
  ensure_event(ln.ev_k);
  if (!ln.h_bad) HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&ln.h_bad), 16, hipHostMallocDefault));
  ln.h_counts32.ensure(cap_q);
  ensure(ln.counts, cap_q);
  ensure(ln.counts32, cap_q);
  ensure(ln.bad, 2);
  return ln;
}

// locate lane li for chunks of up to cap reads: events, range words (rs_words per read), counts, hit offsets and scan scratch,
// the first-bad word, the pinned chunk totals; W != 0: packed words (W per read) on the device and in pinned staging
LocateLane& prepare_locate_lane(Replica& r, int li, uint64_t cap, uint64_t W, int rs_words) {
  LocateLane& ln = r.loc_lanes[li];
  ensure_event(ln.counted);
  ensure_event(ln.located);
  ensure_event(ln.ev_in);
  ensure_event(ln.ev_k);
  if (W) { ensure(ln.words, cap * W); ln.h_words.ensure(cap * W); }
  ensure(ln.rstart, rs_words * cap);
  ensure(ln.counts, cap);
  ensure(ln.hit_off, cap + 1);
  ensure(ln.scratch, scan_tiles(cap) + 1);
  ensure(ln.bad, 2);
  ln.h_meta.ensure(3);
  return ln;
}

// The queries of chunk [lo, lo + n) with letters outside ACGT (`bad`: their indices in the chunk) travel as a compact CSR
// batch of their own -- indices, offsets, bytes, staged in the lane's pinned buffers -- and are redone on `s` by the generic
// kernel (LIST_COMPACT), which overwrites their packed counts and, with d_rstart, their range words (starts only, the packed
// kernels' layout), and leaves the lowest query it rejects in ln.bad[1]: results never depend on the path.
// reset_first_bad: ln.bad[1] is set to "none" here, in front of the kernel (the locate pipeline does it at the head of a chunk).
template <class Lane>
void stage_listed_reads(Replica& r, Lane& ln, hipStream_t s, const uint8_t* qbytes, const uint64_t* qoff, uint64_t lo, uint64_t n,
                        const std::vector<uint32_t>& bad, uint64_t* d_rstart, bool reset_first_bad) {
  const uint64_t nb = bad.size();
  ln.h_bq.ensure(nb);
  ln.h_boff.ensure(nb + 1);
  uint64_t tot = 0;
  for (uint64_t i = 0; i < nb; i++) {
    const uint64_t q = lo + bad[i];
    ln.h_bq.p[i] = bad[i];
    ln.h_boff.p[i] = tot;
    tot += qoff[q + 1] - qoff[q];
  }
  ln.h_boff.p[nb] = tot;
  ln.h_bbytes.ensure(tot + 16);
  HostPool::instance().run_ranges(nb, 4096, [&](uint64_t x, uint64_t y) {
    for (uint64_t i = x; i < y; i++) {
      const uint64_t q = lo + bad[i];
      memcpy(ln.h_bbytes.p + ln.h_boff.p[i], qbytes + qoff[q], qoff[q + 1] - qoff[q]);
    }
  });
  if (ln.bad_list.n < nb) ln.bad_list.alloc(nb + nb / 4 + 1024);
  if (ln.boff.n < nb + 1) ln.boff.alloc(nb + nb / 4 + 1024);
  if (ln.bbytes.n < tot + 16) ln.bbytes.alloc(tot + tot / 4 + 4096);
  HIP_CHECK(hipMemcpyAsync(ln.bad_list.p, ln.h_bq.p, nb * 4, hipMemcpyHostToDevice, s));
  HIP_CHECK(hipMemcpyAsync(ln.boff.p, ln.h_boff.p, (nb + 1) * 8, hipMemcpyHostToDevice, s));
  HIP_CHECK(hipMemcpyAsync(ln.bbytes.p, ln.h_bbytes.p, tot, hipMemcpyHostToDevice, s));
  if (reset_first_bad) HIP_CHECK(hipMemsetAsync(ln.bad.p + 1, 0xFF, 8, s));
  const QueryList ql{ln.bad_list.p, nullptr, nb, nullptr, ln.bad.p + 1, d_rstart ? 1u : 0u};
  hipLaunchKernelGGL((count_scalar_kernel<NUCLEOTIDE, LIST_COMPACT>), dim3(grid_for(r, nb, 256)), dim3(256), 0, s, r.dev, ln.bbytes.p, ln.boff.p, n,
                     ln.counts.p, d_rstart, nullptr, 1, 0, ql);
  HIP_CHECK(hipGetLastError());
}

// The end of a chunk on a count lane: its n counts narrowed to 32-bit words where they fit (narrow32: a count is at most
// bwt_len), then copied into the lane's pinned staging on `cout` -- the lane's own stream, or the replica's copy-out stream
// behind everything the lane stream holds for this chunk.  64-bit counts are staged in h_words.  The caller records ln.done.
void enqueue_counts_out(Replica& r, PackedLane& ln, uint64_t n, bool narrow32, hipStream_t cout) {
  if (narrow32) {
    hipLaunchKernelGGL(narrow_counts_kernel, dim3(grid_for(r, n, 1024)), dim3(256), 0, ln.s, ln.counts.p, ln.counts32.p, n);
    HIP_CHECK(hipGetLastError());
  }
  if (cout != ln.s) {
    HIP_CHECK(hipEventRecord(ln.ev_k, ln.s));
    HIP_CHECK(hipStreamWaitEvent(cout, ln.ev_k, 0));
  }
  if (narrow32) HIP_CHECK(hipMemcpyAsync(ln.h_counts32.p, ln.counts32.p, n * 4, hipMemcpyDeviceToHost, cout));
  else HIP_CHECK(hipMemcpyAsync(ln.h_words.p, ln.counts.p, n * 8, hipMemcpyDeviceToHost, cout));
}

// Retirement of a count lane's chunk: wait for it, spread its counts into counts_out on the pool (the first-touch faults of
// a fresh result array are taken by all threads), raise INVALID_QUERY for the lowest query of the chunk that the reference
// leaves undefined (ln.h_bad[1]).  t_wait / t_out: milliseconds, accumulated for AWRY_TRACE_HOST.
void retire_count_lane(PackedLane& ln, uint64_t* counts_out, bool narrow32, double& t_wait, double& t_out) {
  if (!ln.busy) return;
  ln.busy = false;
  const auto a = std::chrono::steady_clock::now();
  HIP_CHECK(hipEventSynchronize(ln.done));
  const auto b = std::chrono::steady_clock::now();
  const uint64_t n = ln.chunk_hi - ln.chunk_lo;
  if (narrow32) pool_widen_u32(counts_out + ln.chunk_lo, ln.h_counts32.p, n);
  else pool_memcpy(counts_out + ln.chunk_lo, ln.h_words.p, n * 8);  // (a count may pass 2^32: 64-bit words, staged where the packed words were)
  t_wait += std::chrono::duration<double, std::milli>(b - a).count();
  t_out += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - b).count();
  raise_first_bad(ln.h_bad[1], ln.chunk_lo);
}

// The packed lanes with HOST packing -- the default path of parallel_count for nucleotide batches.  Per chunk: the pool
// packs the ASCII into the lane's pinned staging (2 bits per letter: 8 B per 31-mer cross PCIe instead of 31 B, and no
// caller memory is ever registered with the driver -- hipHostRegister of a fresh 150 MB batch cost more than its
// transfer), H2D, packed kernels, D2H of the counts into pinned staging, and on retirement a pool memcpy into
// counts_out (the first-touch faults of a fresh result array are taken by all threads).  The few queries with letters
// outside ACGT travel as a compact CSR batch of their own and are redone on the device by the generic kernel
// (LIST_COMPACT), overwriting their packed counts: results never depend on the path.
// words != nullptr: the caller's k-mers are packed already (awry_count_packed_kmers): staged with a pool memcpy.
// A caller that allocates its result array per call (a fresh Vec<u64>) hands over untouched pages: filling 40 MB of them
// costs ~10 000 page faults.  Advising huge pages for the 2 MB-aligned interior makes that ~20 (no effect where the pages
// are already there, or where transparent huge pages are off); the advice is the only thing done to the caller's mapping.
void advise_huge_pages(void* p, size_t bytes) {
  static const bool off = getenv("AWRY_NO_THP_ADVICE") != nullptr;
  if (off || bytes < (8u << 20)) return;
  const uintptr_t a = (reinterpret_cast<uintptr_t>(p) + (2u << 20) - 1) & ~(uintptr_t)((2u << 20) - 1);
  const uintptr_t b = (reinterpret_cast<uintptr_t>(p) + bytes) & ~(uintptr_t)((2u << 20) - 1);
  if (b > a) (void)madvise(reinterpret_cast<void*>(a), b - a, MADV_HUGEPAGE);
}

struct NotUniform {};  // thrown by count_shard_hostpacked(assume_uniform) when a query's length differs from the assumed one
void count_shard_hostpacked(Replica& r, const uint8_t* qbytes, const uint64_t* qoff, Shard sh, PackedPlan plan, uint64_t* counts_out,
                            const uint64_t* words = nullptr, bool assume_uniform = false) {
  const uint64_t L = plan.Lmax, W = (L + 31) / 32;
  static const bool trace = getenv("AWRY_TRACE_HOST") != nullptr;
  static const uint64_t chunk_q = [] { const char* e = getenv("AWRY_HOST_CHUNK"); return e && atoll(e) > 0 ? (uint64_t)atoll(e) : (uint64_t)(1u << 20); }();
  // full-size chunks, then a tail that halves down to 128 K queries: what cannot overlap anything is the GPU time of
  // the last chunk, so it is kept small
  std::vector<Shard> chunks;
  for (uint64_t a = sh.lo; a < sh.hi;) {
    const uint64_t rest = sh.hi - a;
    uint64_t m = std::min(chunk_q, std::max<uint64_t>(rest / 2, std::min<uint64_t>(rest, 128u << 10)));
    if (rest - m < (64u << 10)) m = rest;
    if (!words && qoff[a + m] - qoff[a] > (256ull << 20)) {  // long reads: bound the bytes too
      m = (uint64_t)(std::upper_bound(qoff + a, qoff + a + m + 1, qoff[a] + (256ull << 20)) - qoff) - 1 - a;
      m = std::max<uint64_t>(m, 1);
    }
    chunks.push_back(Shard{a, a + m});
    a += m;
  }
  uint64_t cap_q = 0;
  for (Shard c : chunks) cap_q = std::max(cap_q, c.hi - c.lo);
  auto now = [] { return std::chrono::steady_clock::now(); };
  auto ms = [](auto a, auto b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
  double t_pack = 0, t_wait = 0, t_out = 0, t_bad = 0;
  double t_enq[5] = {0, 0, 0, 0, 0};  // enqueue by operation: copy in, count kernels, listed reads, narrow + copy out, event
  const bool narrow32 = r.dev.bwt_len < (1ull << 32);  // a count is at most bwt_len
  advise_huge_pages(counts_out + sh.lo, (sh.hi - sh.lo) * 8);
  std::lock_guard<std::mutex> lane_lock(r.lane_mu);
  const auto t0 = now();
  PackedLane* lanes = r.lanes;
  uint64_t redone = 0;
  auto retire = [&](PackedLane& ln) {
    if (ln.busy) redone += ln.nbad;
    retire_count_lane(ln, counts_out, narrow32, t_wait, t_out);
  };
  DrainLanes drain{r};
  const int nl = (int)std::min<size_t>(Replica::NLANES, chunks.size());
  for (int li = 0; li < nl; li++) {
    PackedLane& ln = prepare_count_lane(r, li, cap_q);
    ln.h_words.ensure(cap_q * W);
    ensure(ln.words, cap_q * W);
    if (plan.ragged) { ln.h_lens.ensure(cap_q); ensure(ln.lens, cap_q); }
  }
  const auto t1 = now();
  std::vector<uint32_t> bad;
  int which = 0;
  for (Shard c : chunks) {
    PackedLane& ln = lanes[which];
    which = (which + 1) % nl;
    retire(ln);
    const uint64_t lo = c.lo, hi = c.hi, n = hi - lo;
    ln.chunk_lo = lo;
    ln.chunk_hi = hi;
    auto a = now();
    if (words) { pool_memcpy(ln.h_words.p, words + lo, n * 8); bad.clear(); }
    // (assume_uniform: the chunks before this one have been checked, so qoff[lo] is where query lo starts either way)
    else if (!pack_nt2_host(qbytes + qoff[lo], qbytes + qoff[sh.hi], plan.ragged ? qoff : nullptr, lo, hi, L, ln.h_words.p,
                            plan.ragged ? ln.h_lens.p : nullptr, bad, assume_uniform ? qoff : nullptr))
      throw NotUniform{};  // (DrainLanes leaves the lanes idle; the caller plans the batch again from a full length scan)
    auto b = now();
    ln.nbad = bad.size();
    if (!ln.nbad) ln.h_bad[1] = ~0ull;  // (no listed queries: nothing writes the lane's first-bad word, and retirement reads it)
    // (the lane's previous chunk has been retired: its kernels and its copy out are done, ln.words / ln.counts32 are free)
    // the chunk copies go through the replica's copy streams (see Replica::copy_in), tied to the lane's kernels by events
    hipStream_t cin = r.copy_in, cout = r.copy_out;
    HIP_CHECK(hipMemcpyAsync(ln.words.p, ln.h_words.p, n * W * 8, hipMemcpyHostToDevice, cin));
    if (plan.ragged) HIP_CHECK(hipMemcpyAsync(ln.lens.p, ln.h_lens.p, n * 4, hipMemcpyHostToDevice, cin));
    HIP_CHECK(hipEventRecord(ln.ev_in, cin));
    HIP_CHECK(hipStreamWaitEvent(ln.s, ln.ev_in, 0));
    auto e1 = now();
    if (L <= 32 && !plan.ragged) launch_count_nt2(r, ln.words.p, n, (int)L, ln.counts.p, true, ln.s, nullptr);
    else launch_count_nt2_long(r, ln.words.p, n, (int)L, ln.counts.p, nullptr, true, ln.s, plan.ragged ? ln.lens.p : nullptr);
    auto e2 = now();
    if (ln.nbad) {
      stage_listed_reads(r, ln, ln.s, qbytes, qoff, lo, n, bad, nullptr, true);
      HIP_CHECK(hipMemcpyAsync(ln.h_bad + 1, ln.bad.p + 1, 8, hipMemcpyDeviceToHost, ln.s));
    }
    auto e3 = now();
    enqueue_counts_out(r, ln, n, narrow32, cout);
    auto e4 = now();
    HIP_CHECK(hipEventRecord(ln.done, cout));
    ln.busy = true;
    if (trace) {
      t_pack += ms(a, b); t_bad += ms(b, now());
      t_enq[0] += ms(b, e1); t_enq[1] += ms(e1, e2); t_enq[2] += ms(e2, e3); t_enq[3] += ms(e3, e4); t_enq[4] += ms(e4, now());
    }
  }
  for (int k = 0; k < nl; k++) { retire(lanes[which]); which = (which + 1) % nl; }  // in chunk order
  if (trace)
    fprintf(stderr, "[awry] host-packed shard %llu queries%s L=%llu, %zu chunks, %u pool threads: lane setup %.2f ms, pipeline %.2f ms (%s %.2f, enqueue %.2f "
            "[copy in %.2f, count kernels %.2f, listed reads %.2f, narrow + copy out %.2f, event %.2f], "
            "waiting for the GPU %.2f, copying counts out %.2f), %llu redone by the generic kernel\n",
            (unsigned long long)(sh.hi - sh.lo), plan.ragged ? " (ragged)" : "", (unsigned long long)L, chunks.size(), HostPool::instance().threads(),
            ms(t0, t1), ms(t1, now()), words ? "staging" : "host pack", t_pack, t_bad, t_enq[0], t_enq[1], t_enq[2], t_enq[3], t_enq[4], t_wait, t_out,
            (unsigned long long)redone);
}

// Generic kernel, pipelined like the packed path: any alphabet, any letters, any lengths (amino batches, long or very
// unequal nucleotide reads).  Pinned input / offsets / output, two stream lanes, persistent lane buffers; the kernel
// reads the chunk's queries through the batch's own offsets (the ASCII pointer is biased by the chunk's first byte).
// ulen != 0: every query of the shard has ulen bytes -- the offsets stay on the host and the kernels address query q at q * ulen.
void count_shard_generic_pipelined(Replica& r, const uint8_t* qbytes, const uint64_t* qoff, Shard sh, uint64_t* counts_out, uint64_t ulen = 0) {
  if (!ulen)  // (one length: the length scan has seen every offset already)
    for (uint64_t i = sh.lo; i < sh.hi; i++)  // (vectorises) non-decreasing offsets
      if (qoff[i + 1] < qoff[i]) throw ArgError("query offsets must be non-decreasing");
  const std::vector<Shard> chunks = packed_chunks(qoff, sh, 1u << 20, 128ull << 20);
  uint64_t cap_q = 0, cap_b = 0;
  for (Shard c : chunks) { cap_q = std::max(cap_q, c.hi - c.lo); cap_b = std::max(cap_b, qoff[c.hi] - qoff[c.lo]); }
  std::lock_guard<std::mutex> lane_lock(r.lane_mu);
  static const bool trace = getenv("AWRY_TRACE_HOST") != nullptr;
  const auto t0 = std::chrono::steady_clock::now();
  // Like the host-packed lanes: the chunk's bytes (and offsets) are copied by the pool into the lane's pinned staging --
  // nothing of the caller's is registered with the driver --, counts come back as 32-bit words when they fit (a count is
  // at most bwt_len) and are widened into counts_out, and instead of one status byte per query the lowest rejected
  // query crosses PCIe as one word.
  const bool narrow32 = r.dev.bwt_len < (1ull << 32);
  PackedLane* lanes = r.lanes;
  double t_stage = 0, t_wait = 0, t_out = 0;
  auto now = [] { return std::chrono::steady_clock::now(); };
  auto ms = [](auto a, auto b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
  auto retire = [&](PackedLane& ln) { retire_count_lane(ln, counts_out, narrow32, t_wait, t_out); };
  DrainLanes drain{r};
  const int nl = (int)std::min<size_t>(Replica::NLANES, chunks.size());
  for (int li = 0; li < nl; li++) {
    PackedLane& ln = prepare_count_lane(r, li, cap_q);
    ln.h_bbytes.ensure(cap_b + 16);
    ensure(ln.ascii, cap_b + 16);
    if (!ulen) { ln.h_boff.ensure(cap_q + 1); ensure(ln.off, cap_q + 1); }
    ensure(ln.status, cap_q);
    if (!narrow32) ln.h_words.ensure(cap_q);  // (pinned staging of the 64-bit counts)
  }
  int which = 0;
  for (Shard c : chunks) {
    PackedLane& ln = lanes[which];
    which = (which + 1) % nl;
    retire(ln);
    const uint64_t lo = c.lo, hi = c.hi, n = hi - lo, base = qoff[lo], nbytes = qoff[hi] - base;
    ln.chunk_lo = lo;
    ln.chunk_hi = hi;
    auto a = now();
    if (nbytes) pool_memcpy(ln.h_bbytes.p, qbytes + base, nbytes);
    if (!ulen) pool_memcpy(ln.h_boff.p, qoff + lo, (n + 1) * 8);
    if (trace) t_stage += ms(a, now());
    if (nbytes) HIP_CHECK(hipMemcpyAsync(ln.ascii.p, ln.h_bbytes.p, nbytes, hipMemcpyHostToDevice, ln.s));
    if (ulen) {
      launch_count_ascii_uniform(r, ln.ascii.p, n, ulen, ln.counts.p, ln.status.p, ln.s);
    } else {
      HIP_CHECK(hipMemcpyAsync(ln.off.p, ln.h_boff.p, (n + 1) * 8, hipMemcpyHostToDevice, ln.s));
      const uint8_t* biased = reinterpret_cast<const uint8_t*>(reinterpret_cast<uintptr_t>(ln.ascii.p) - base);
      launch_count_ascii(r, biased, ln.off.p, n, ln.counts.p, nullptr, ln.status.p, ln.s, true);
    }
    HIP_CHECK(hipMemsetAsync(ln.bad.p + 1, 0xFF, 8, ln.s));
    hipLaunchKernelGGL(status_first_bad_kernel, dim3(grid_for(r, n, 4096)), dim3(256), 0, ln.s, ln.status.p, n, ln.bad.p + 1);
    HIP_CHECK(hipGetLastError());
    enqueue_counts_out(r, ln, n, narrow32, ln.s);  // (this pipeline copies on its lane streams)
    HIP_CHECK(hipMemcpyAsync(ln.h_bad + 1, ln.bad.p + 1, 8, hipMemcpyDeviceToHost, ln.s));
    HIP_CHECK(hipEventRecord(ln.done, ln.s));
    ln.busy = true;
  }
  for (int k2 = 0; k2 < nl; k2++) { retire(lanes[which]); which = (which + 1) % nl; }
  if (trace)
    fprintf(stderr, "[awry] generic shard %llu queries%s, %zu chunks: %.2f ms (staging %.2f, waiting for the GPU %.2f, copying counts out %.2f)\n",
            (unsigned long long)(sh.hi - sh.lo), ulen ? " (one length)" : "", chunks.size(), ms(t0, now()), t_stage, t_wait, t_out);
}

void count_shard_generic(Replica& r, const uint8_t* qbytes, const uint64_t* qoff, Shard sh, uint64_t* counts_out) {
  HIP_CHECK(hipSetDevice(r.device));
  ChunkBuffers cb;
  for (Shard c : chunk_queries(qoff, sh.lo, sh.hi)) {
    run_count_chunk(r, cb, qbytes, qoff, c, false);
    HIP_CHECK(hipMemcpyAsync(counts_out + c.lo, cb.counts.p, (c.hi - c.lo) * 8, hipMemcpyDeviceToHost, r.stream));
    HIP_CHECK(hipStreamSynchronize(r.stream));
    check_status(cb, c.lo);
  }
}

void count_shard(Replica& r, const uint8_t* qbytes, const uint64_t* qoff, Shard sh, uint64_t* counts_out) {
  HIP_CHECK(hipSetDevice(r.device));
  static const bool no_fast = getenv("AWRY_HOST_PATH") && !strcmp(getenv("AWRY_HOST_PATH"), "generic");
  const auto t0 = std::chrono::steady_clock::now();
  PackedPlan plan;
  const bool packable = !no_fast && r.dev.alphabet == NUCLEOTIDE;  // (wide-row replicas take the 64-bit packed kernels)
  if (packable && sh.hi - sh.lo >= (1u << 16)) {
    // k-mer and read batches are nearly always of one length: assume the first query's, let the packer check the
    // offsets in the pass that reads the bytes anyway (a separate scan of 8 B per query costs 7 % of a 31-mer batch)
    const uint64_t n = sh.hi - sh.lo, L0 = qoff[sh.lo + 1] - qoff[sh.lo];
    if (L0 >= 1 && L0 <= 4096 && qoff[sh.hi] >= qoff[sh.lo] && qoff[sh.hi] - qoff[sh.lo] == n * L0) {
      PackedPlan guess;
      guess.ok = true;
      guess.Lmax = L0;
      try {
        count_shard_hostpacked(r, qbytes, qoff, sh, guess, counts_out, nullptr, true);
        return;
      } catch (const NotUniform&) {  // plan it properly below; what was written to counts_out is overwritten
      }
    }
  }
  if (packable) plan = plan_packed(qoff, sh);
  if (getenv("AWRY_TRACE_HOST"))
    fprintf(stderr, "[awry] length scan %.2f ms\n", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
  if (plan.ok) {
    count_shard_hostpacked(r, qbytes, qoff, sh, plan, counts_out);
    return;
  }
  if (!no_fast && sh.hi - sh.lo >= 4096) {
    // amino batches of one length (k-mers): no offsets cross PCIe and the two-phase amino schedule serves them
    uint64_t ulen = 0;
    if (r.dev.alphabet == AMINO) {
      const PackedPlan ap = plan_packed(qoff, sh);
      if (ap.ok && !ap.ragged) ulen = ap.Lmax;
      if (getenv("AWRY_TRACE_HOST"))
        fprintf(stderr, "[awry] amino length scan %.2f ms\n", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    }
    count_shard_generic_pipelined(r, qbytes, qoff, sh, counts_out, ulen);
  } else count_shard_generic(r, qbytes, qoff, sh, counts_out);
}

// run fn(replica, shard, slot) on every replica concurrently; rethrow the first failure
template <class F>
void for_each_replica(awry_index* ix, uint64_t n, F&& fn) {
  if (ix->reps.empty()) throw NoDeviceError("no device replica: call awry_set_devices() first (there is no CPU search path)");
  auto shards = shard_queries(n, ix->reps.size());
  if (ix->reps.size() == 1) { fn(*ix->reps[0], shards[0], 0); return; }
  std::vector<std::exception_ptr> errs(ix->reps.size());
  std::vector<std::thread> pool;
  for (size_t g = 0; g < ix->reps.size(); g++)
    pool.emplace_back([&, g] {
      try { fn(*ix->reps[g], shards[g], (int)g); } catch (...) { errs[g] = std::current_exception(); }
    });
  for (auto& t : pool) t.join();
  for (auto& e : errs) if (e) std::rethrow_exception(e);
}

}  // namespace
