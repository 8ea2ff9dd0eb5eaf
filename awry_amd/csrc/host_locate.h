// host_locate.h -- pinned result arrays and the locate pipelines
// A part of awry_hip.hip (one translation unit): included there, in order, and not on its own.
#pragma once

namespace {

// Result arrays of the batch entry points (offsets, positions, (record, offset) pairs) are PINNED host memory, recycled
// through a process-wide pool: the locate kernels' output is copied by the DMA engine straight into the array the caller
// receives -- no pinned staging, no host memcpy, and after the first call no first-touch page faults either (a fresh
// 100 MB array costs more in faults than its bytes cost on PCIe).  awry_free_buffer returns a block to the pool; blocks
// are kept up to AWRY_PINNED_CACHE_GB (default 4) and otherwise released.  Where pinning fails the arrays are plain
// malloc memory and the copies are staged by the runtime.
class PinnedPool {
 public:
  static PinnedPool& instance() {
    static PinnedPool* pool = new PinnedPool;  // never destroyed: the HIP runtime may be gone before static destructors run
    return *pool;
  }
  void* get(size_t bytes) {  // >= bytes of pinned memory, or nullptr
    const size_t want = round_up(bytes);
    {
      std::lock_guard<std::mutex> lk(mu_);
      auto it = free_.lower_bound(want);
      if (it != free_.end() && it->first <= 2 * want) {
        void* p = it->second;
        cached_ -= it->first;
        live_[p] = it->first;
        free_.erase(it);
        return p;
      }
    }
    void* p = nullptr;
    if (hipHostMalloc(&p, want, hipHostMallocPortable) != hipSuccess || !p) { (void)hipGetLastError(); return nullptr; }
    std::lock_guard<std::mutex> lk(mu_);
    live_[p] = want;
    return p;
  }
  bool put(void* p) {  // false: not a block of this pool
    size_t bytes = 0;
    {
      std::lock_guard<std::mutex> lk(mu_);
      auto it = live_.find(p);
      if (it == live_.end()) return false;
      bytes = it->second;
      live_.erase(it);
      if (cached_ + bytes <= cap_) {
        free_.emplace(bytes, p);
        cached_ += bytes;
        return true;
      }
    }
    (void)hipHostFree(p);
    return true;
  }
 private:
  PinnedPool() {
    const char* e = getenv("AWRY_PINNED_CACHE_GB");
    cap_ = (size_t)((e && atof(e) >= 0 ? atof(e) : 4.0) * (double)(1ull << 30));
  }
  static size_t round_up(size_t b) {  // 1 MiB, then powers of two up to 64 MiB, then multiples of 64 MiB
    size_t c = 1u << 20;
    while (c < b && c < (64u << 20)) c <<= 1;
    return c >= b ? c : (b + (64u << 20) - 1) / (64u << 20) * (64u << 20);
  }
  std::mutex mu_;
  std::multimap<size_t, void*> free_;
  std::map<void*, size_t> live_;
  size_t cached_ = 0, cap_ = 0;
};

void release_result(void* p) {
  if (p && !PinnedPool::instance().put(p)) free(p);
}

template <class T>
struct MBuf {  // geometrically growing result array whose storage is handed to the caller (released with awry_free_buffer)
  T* p = nullptr;
  size_t cap = 0;
  size_t used_bytes = 0;  // bytes of p[] that hold data (what a re-allocation has to carry over)
  MBuf() = default;
  MBuf(const MBuf&) = delete;
  MBuf& operator=(const MBuf&) = delete;
  MBuf(MBuf&& o) noexcept : p(o.p), cap(o.cap), used_bytes(o.used_bytes) { o.p = nullptr; o.cap = 0; o.used_bytes = 0; }
  ~MBuf() { release_result(p); }
  void grow(size_t need) {
    if (need <= cap) return;
    const size_t c = std::max(need, cap + cap / 2 + 4096), bytes = c * sizeof(T);
    void* q = bytes >= (256u << 10) ? PinnedPool::instance().get(bytes) : nullptr;
    if (!q) q = malloc(bytes);
    if (!q) throw std::bad_alloc();
    if (p && used_bytes) pool_memcpy(q, p, used_bytes);
    release_result(p);
    p = static_cast<T*>(q);
    cap = c;
  }
  T* release() { T* q = p; p = nullptr; cap = 0; used_bytes = 0; return q; }
};

struct LocateResult {  // per shard, in query order
  uint64_t* off = nullptr;  // the shard's slice of the batch's offset array: off[i + 1] - off[i] = hits of query i; the
                            //   shard writes off[1..n] relative to its own first hit, the caller rebases
  uint64_t nq = 0, filled = 0, running = 0;
  MBuf<uint64_t> gpos;
  MBuf<awry_pos_t> pos;
  size_t total = 0;      // hits whose results are in (or on their way into) the arrays
  bool want_pos = true;  // false: the caller passed hits_out == NULL -- (record, offset) pairs are neither computed nor moved
  void add_counts(const uint64_t* counts, uint64_t n) {  // next n queries of the shard
    for (uint64_t i = 0; i < n; i++) { running += counts[i]; off[filled + i + 1] = running; }
    filled += n;
  }
  // next n queries of the shard, whose inclusive hit offsets RELATIVE TO THE CHUNK already sit in off[filled + 1 ...]
  // (copied there from the device scan): rebase them onto the shard's running total
  void rebase_offsets(uint64_t n, uint64_t chunk_total) {
    uint64_t* o = off + filled + 1;
    const uint64_t base = running;
    if (base) HostPool::instance().run_ranges(n, 1u << 16, [&](uint64_t a, uint64_t b) { for (uint64_t i = a; i < b; i++) o[i] += base; });
    running += chunk_total;
    filled += n;
  }
  // room for n more hits; true when an array moved (copies in flight into the old one must have finished: see `quiesce`)
  template <class Quiesce>
  void reserve(size_t n, bool want_gpos, Quiesce&& quiesce) {
    if ((!want_pos || total + n <= pos.cap) && (!want_gpos || total + n <= gpos.cap)) return;
    size_t need = total + n;
    if (filled && filled < nq) need = std::max(need, (size_t)((double)(total + n) / (double)filled * (double)nq * 1.05) + 4096);  // the whole shard, from the hit rate so far
    quiesce();
    if (want_pos) { pos.used_bytes = total * sizeof(awry_pos_t); pos.grow(need); }
    if (want_gpos) { gpos.used_bytes = total * 8; gpos.grow(need); }
  }
  void append(const uint64_t* g, const awry_pos_t* p, size_t n, bool want_gpos) {
    if (!n) return;
    reserve(n, want_gpos, [] {});
    if (want_pos) pool_memcpy(pos.p + total, p, n * sizeof(awry_pos_t));
    if (want_gpos) pool_memcpy(gpos.p + total, g, n * 8);
    total += n;
  }
};

// generic kernels, synchronous: any alphabet, ragged lengths, ambiguity codes
void locate_chunk_generic(Replica& r, const uint8_t* qbytes, const uint64_t* qoff, Shard c, uint64_t* counts_out,
                          std::vector<uint64_t>& gpos, std::vector<awry_pos_t>& pos, bool want_pos) {
  ChunkBuffers cb;
  const uint64_t n = c.hi - c.lo;
  run_count_chunk(r, cb, qbytes, qoff, c, true);
  DevBuf<uint64_t> hit_off(n + 1), scratch(scan_tiles(n) + 1);
  launch_scan(r, cb.counts.p, n, hit_off.p, scratch.p, r.stream);
  uint64_t total = 0;
  HIP_CHECK(hipMemcpyAsync(&total, hit_off.p + n, 8, hipMemcpyDeviceToHost, r.stream));
  HIP_CHECK(hipMemcpyAsync(counts_out, cb.counts.p, n * 8, hipMemcpyDeviceToHost, r.stream));
  HIP_CHECK(hipStreamSynchronize(r.stream));
  check_status(cb, c.lo);
  gpos.resize(total);
  pos.resize(want_pos ? total : 0);
  if (total == 0) return;
  DevBuf<uint64_t> d_gpos(total), d_pos(want_pos ? 2 * total : 0);
  launch_locate(r, cb.ranges.p, 2, hit_off.p, n, total, d_gpos.p, d_pos.p, r.stream);
  if (want_pos) HIP_CHECK(hipMemcpyAsync(pos.data(), d_pos.p, total * 16, hipMemcpyDeviceToHost, r.stream));
  HIP_CHECK(hipMemcpyAsync(gpos.data(), d_gpos.p, total * 8, hipMemcpyDeviceToHost, r.stream));
  HIP_CHECK(hipStreamSynchronize(r.stream));
}

void locate_shard_generic(Replica& r, const uint8_t* qbytes, const uint64_t* qoff, Shard sh, bool want_gpos, LocateResult& out) {
  std::vector<uint64_t> g, counts;
  std::vector<awry_pos_t> p;
  for (Shard c : chunk_queries(qoff, sh.lo, sh.hi)) {
    counts.resize(c.hi - c.lo);
    locate_chunk_generic(r, qbytes, qoff, c, counts.data(), g, p, out.want_pos);
    out.add_counts(counts.data(), c.hi - c.lo);
    out.append(g.data(), p.data(), g.size(), want_gpos);
  }
}

// Fast path of parallel_locate: nucleotide index, every read the same length L.  Chunks of reads flow through the
// replica's two stream lanes in three stages -- (1) H2D ASCII, pack, packed count with range starts, scan, D2H counts;
// (2) once the host knows the chunk's hit total: locate kernels, D2H of the positions into pinned staging; (3) copy
// into the result arrays -- so that one chunk's transfers and host copies overlap the other chunk's kernels.  A chunk
// that holds bytes outside ACGT is redone by the generic kernels; results never depend on the path.
// plan.ok == false: the same pipeline around the generic kernel (any alphabet, letters and lengths; ranges as two words
// per query, statuses checked in stage 2)
void locate_shard_packed(Replica& r, const uint8_t* qbytes, const uint64_t* qoff, Shard sh, PackedPlan plan, bool want_gpos, LocateResult& out) {
  const bool generic = !plan.ok, want_pos = out.want_pos;
  uint64_t ulen = 0;  // generic, every query of one length (amino k-mers): no offsets travel, the amino k-mer schedule counts
  if (generic) {
    if (r.dev.alphabet == AMINO) {
      const PackedPlan ap = plan_packed(qoff, sh);
      if (ap.ok && !ap.ragged) ulen = ap.Lmax;
    }
    plan.ragged = ulen == 0;  // offsets travel with the chunk
    plan.Lmax = 1;
    if (!ulen)
      for (uint64_t i = sh.lo; i < sh.hi; i++)
        if (qoff[i + 1] < qoff[i]) throw ArgError("query offsets must be non-decreasing");
  }
  const uint64_t L = plan.Lmax, W = (L + 31) / 32;
  // nucleotide reads are packed on the HOST (2 bits per letter cross PCIe, nothing of the caller's is registered with the
  // driver), as in count_shard_hostpacked; the generic pipeline copies the caller's bytes from where they lie, registered in place
  const std::vector<Shard> chunks = packed_chunks(qoff, sh, 1u << 20, 128ull << 20);
  uint64_t cap = 0, cap_b = 0;
  for (Shard c : chunks) { cap = std::max(cap, c.hi - c.lo); cap_b = std::max(cap_b, qoff[c.hi] - qoff[c.lo]); }
  static const bool trace = getenv("AWRY_TRACE_HOST") != nullptr;
  const auto t0 = std::chrono::steady_clock::now();
  std::lock_guard<std::mutex> lane_lock(r.lane_mu);
  HostPin pin_in(generic ? qbytes + qoff[sh.lo] : nullptr, qoff[sh.hi] - qoff[sh.lo]);
  HostPin pin_off(plan.ragged && generic ? qoff + sh.lo : nullptr, (sh.hi - sh.lo + 1) * 8);
  std::vector<uint32_t> bad;
  double t_pack = 0;
  LocateLane* lanes = r.loc_lanes;
  double t_pin = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(), t_wait_count = 0, t_wait_locate = 0;
  double t_grow_host = 0, t_grow_dev = 0;  // result arrays (pinned pool) and the lanes' device hit buffers that had to grow
  int n_grow_host = 0, n_grow_dev = 0;
  auto timed = [&](double& acc, auto&& fn) {
    if (!trace) { fn(); return; }
    const auto a = std::chrono::steady_clock::now();
    fn();
    acc += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - a).count();
  };
  DrainLanes drain{r};  // (every exit leaves the lanes idle before the input is unpinned)
  // chunk copies on the replica's copy-in / copy-out streams (see Replica::copy_in)
  for (int li = 0; li < 2; li++) {
    LocateLane& ln = prepare_locate_lane(r, li, cap, generic ? 0 : W, generic ? 2 : 1);
    if (plan.ragged && !generic) { ensure(ln.lens, cap); ln.h_lens.ensure(cap); }
    if (generic) {
      ensure(ln.ascii, cap_b + 16);
      if (plan.ragged) ensure(ln.off, cap + 1);
      ensure(ln.status, cap);
      ln.h_status.ensure(cap);
    }
    ln.stage = 0;
  }
  auto stage1 = [&](int li, uint64_t lo, uint64_t hi) {  // count
    LocateLane& ln = lanes[li];
    hipStream_t s = r.lane_stream[li];
    const uint64_t n = hi - lo;
    ln.lo = lo;
    ln.hi = hi;
    const uint64_t nbytes = qoff[hi] - qoff[lo];
    if (!generic) {
      timed(t_pack, [&] {
        pack_nt2_host(qbytes + qoff[lo], qbytes + qoff[sh.hi], plan.ragged ? qoff : nullptr, lo, hi, L, ln.h_words.p, plan.ragged ? ln.h_lens.p : nullptr, bad);
      });
      hipStream_t cin = r.copy_in;
      HIP_CHECK(hipMemcpyAsync(ln.words.p, ln.h_words.p, n * W * 8, hipMemcpyHostToDevice, cin));
      if (plan.ragged) HIP_CHECK(hipMemcpyAsync(ln.lens.p, ln.h_lens.p, n * 4, hipMemcpyHostToDevice, cin));
      HIP_CHECK(hipEventRecord(ln.ev_in, cin));
      HIP_CHECK(hipStreamWaitEvent(s, ln.ev_in, 0));
      HIP_CHECK(hipMemsetAsync(ln.bad.p, 0, 8, s));
      HIP_CHECK(hipMemsetAsync(ln.bad.p + 1, 0xFF, 8, s));
      launch_count_nt2_long(r, ln.words.p, n, (int)L, ln.counts.p, ln.rstart.p, true, s, plan.ragged ? ln.lens.p : nullptr);
      if (!bad.empty()) stage_listed_reads(r, ln, s, qbytes, qoff, lo, n, bad, ln.rstart.p, false);  // (before the scan)
      launch_scan(r, ln.counts.p, n, ln.hit_off.p, ln.scratch.p, s);
      // (the chunk's hit total and offsets stay on the lane stream: the host needs the total to start stage 2, and on the
      // shared copy-out stream it would queue behind the other lane's result arrays)
      HIP_CHECK(hipMemcpyAsync(ln.h_meta.p, ln.hit_off.p + n, 8, hipMemcpyDeviceToHost, s));
      HIP_CHECK(hipMemcpyAsync(ln.h_meta.p + 1, ln.bad.p, 16, hipMemcpyDeviceToHost, s));
      HIP_CHECK(hipMemcpyAsync(out.off + (lo - sh.lo) + 1, ln.hit_off.p + 1, n * 8, hipMemcpyDeviceToHost, s));  // chunk-relative; rebased in stage 2
      HIP_CHECK(hipEventRecord(ln.counted, s));
      ln.stage = 1;
      return;
    }
    HIP_CHECK(hipMemcpyAsync(ln.ascii.p, qbytes + qoff[lo], nbytes, hipMemcpyHostToDevice, s));
    if (plan.ragged) HIP_CHECK(hipMemcpyAsync(ln.off.p, qoff + lo, (n + 1) * 8, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemsetAsync(ln.bad.p, 0, 8, s));
    HIP_CHECK(hipMemsetAsync(ln.bad.p + 1, 0xFF, 8, s));
    const uint8_t* biased = reinterpret_cast<const uint8_t*>(reinterpret_cast<uintptr_t>(ln.ascii.p) - qoff[lo]);
    if (ulen) launch_count_ascii_uniform(r, ln.ascii.p, n, ulen, ln.counts.p, ln.status.p, s, ln.rstart.p);
    else launch_count_ascii(r, biased, ln.off.p, n, ln.counts.p, ln.rstart.p, ln.status.p, s, true);
    HIP_CHECK(hipMemcpyAsync(ln.h_status.p, ln.status.p, n, hipMemcpyDeviceToHost, s));
    launch_scan(r, ln.counts.p, n, ln.hit_off.p, ln.scratch.p, s);
    HIP_CHECK(hipMemcpyAsync(ln.h_meta.p, ln.hit_off.p + n, 8, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(ln.h_meta.p + 1, ln.bad.p, 16, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(out.off + (lo - sh.lo) + 1, ln.hit_off.p + 1, n * 8, hipMemcpyDeviceToHost, s));  // chunk-relative; rebased in stage 2
    HIP_CHECK(hipEventRecord(ln.counted, s));
    ln.stage = 1;
  };
  auto stage2 = [&](int li) {  // locate, once the chunk's hit total is known
    LocateLane& ln = lanes[li];
    if (ln.stage != 1) return;
    hipStream_t s = r.lane_stream[li];
    const uint64_t n = ln.hi - ln.lo;
    timed(t_wait_count, [&] { HIP_CHECK(hipEventSynchronize(ln.counted)); });
    if (generic) {
      uint64_t any = 0;
      for (uint64_t i = 0; i < n; i++) any |= ln.h_status.p[i];  // (vectorises)
      if (any) check_status(ln.h_status.p, n, ln.lo);  // raises INVALID_QUERY naming the first such query
    } else raise_first_bad(ln.h_meta.p[2], ln.lo);  // the lowest read of the chunk that the reference leaves undefined
    ln.total = ln.h_meta.p[0];
    out.rebase_offsets(n, ln.total);  // stage 2 runs in chunk order
    if (ln.total) {
      // the positions go from the device straight into the result arrays (pinned, PinnedPool): no staging, no host copy.
      // An array that has to grow first waits for the copies still on their way into it.
      timed(t_grow_host, [&] {
        out.reserve(ln.total, want_gpos, [&] {
          n_grow_host++;
          for (int l2 = 0; l2 < 2; l2++) HIP_CHECK(hipStreamSynchronize(r.lane_stream[l2]));
          HIP_CHECK(hipStreamSynchronize(r.copy_out));  // (copies on their way into the old arrays)
        });
      });
      timed(t_grow_dev, [&] {
        if (ln.gpos.n < ln.total) { ln.gpos.alloc(ln.total + ln.total / 4); n_grow_dev++; }
        if (want_pos && ln.pos.n < 2 * ln.total) { ln.pos.alloc(2 * (ln.total + ln.total / 4)); n_grow_dev++; }
      });
      launch_locate(r, ln.rstart.p, generic ? 2 : 1, ln.hit_off.p, n, ln.total, ln.gpos.p, want_pos ? ln.pos.p : nullptr, s);
      hipStream_t cout = r.copy_out;
      HIP_CHECK(hipEventRecord(ln.ev_k, s));
      HIP_CHECK(hipStreamWaitEvent(cout, ln.ev_k, 0));
      if (want_pos) HIP_CHECK(hipMemcpyAsync(out.pos.p + out.total, ln.pos.p, ln.total * 16, hipMemcpyDeviceToHost, cout));
      if (want_gpos) HIP_CHECK(hipMemcpyAsync(out.gpos.p + out.total, ln.gpos.p, ln.total * 8, hipMemcpyDeviceToHost, cout));
      out.total += ln.total;
      HIP_CHECK(hipEventRecord(ln.located, cout));
    } else {
      HIP_CHECK(hipEventRecord(ln.located, s));
    }
    ln.stage = 2;
  };
  auto stage3 = [&](int li) {  // results into the output arrays, in chunk order
    LocateLane& ln = lanes[li];
    if (ln.stage != 2) return;
    timed(t_wait_locate, [&] { HIP_CHECK(hipEventSynchronize(ln.located)); });
    ln.stage = 0;
  };
  uint64_t i = 0;
  for (Shard c : chunks) {
    const int li = (int)(i & 1);
    stage3(li);              // chunk i - 2
    stage1(li, c.lo, c.hi);  // chunk i
    stage2(li ^ 1);          // chunk i - 1
    i++;
  }
  const int last = (int)((i + 1) & 1);            // lane of chunk i - 1
  stage3(last ^ 1);                               // chunk i - 2
  stage2(last);
  stage3(last);
  if (trace)
    fprintf(stderr, "[awry] packed locate shard: %llu reads, %zu hits, %.2f ms (pin %.2f, host pack %.2f, waiting for counts %.2f, for positions %.2f, growing the result arrays %.2f in %d step(s), the lanes' device hit buffers %.2f in %d; results land in the caller's arrays by DMA)\n",
            (unsigned long long)(sh.hi - sh.lo), out.total, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(),
            t_pin, t_pack, t_wait_count, t_wait_locate, t_grow_host, n_grow_host, t_grow_dev, n_grow_dev);
}

void locate_shard(Replica& r, const uint8_t* qbytes, const uint64_t* qoff, Shard sh, bool want_gpos, LocateResult& out) {
  HIP_CHECK(hipSetDevice(r.device));
  out.nq = sh.hi - sh.lo;
  static const bool no_fast = getenv("AWRY_HOST_PATH") && !strcmp(getenv("AWRY_HOST_PATH"), "generic");
  PackedPlan plan;
  if (!no_fast && r.dev.alphabet == NUCLEOTIDE) plan = plan_packed(qoff, sh);
  if (plan.ok || (!no_fast && sh.hi - sh.lo >= 4096))
    locate_shard_packed(r, qbytes, qoff, sh, plan, want_gpos, out);
  else
    locate_shard_generic(r, qbytes, qoff, sh, want_gpos, out);
}

}  // namespace
