// prewarm.h -- what awry_set_devices sets up so that the first batch call of a process costs what the third does
// A part of awry_hip.hip (one translation unit): included there, in order, and not on its own.
#pragma once

namespace {

// The first batch call of a process used to pay for what every later one finds in place: the lanes' pinned staging and device
// buffers, their events, the worker pool's threads and the pinned result arrays of the locate path (4 M 101-bp reads: 30 ms
// for the first awry_locate_batch, 6 ms from the third on).  awry_set_devices sets all of it up for the chunk sizes the
// host paths use (2^20 queries of up to 128 letters), so that call #1 costs what call #3 does.  AWRY_PREWARM=0 skips it.
void prewarm_host_paths(Replica& r) {
  static const bool off = getenv("AWRY_PREWARM") && !strcmp(getenv("AWRY_PREWARM"), "0");
  if (off) return;
  HIP_CHECK(hipSetDevice(r.device));
  // (warm-ups, not a caller's batches of k-mers: they neither build nor find a k-mer count table -- with awry_set_kmer_table(1)
  // inherited by a new replica, the 64 k-mers of length k + 1 of the count lanes' round trip below used to build one)
  struct TableOff { Replica& r; int mode; ~TableOff() { r.kt_mode = mode; } } table_off{r, r.kt_mode};
  r.kt_mode = 0;
  (void)HostPool::instance();
  const bool nt = r.dev.alphabet == NUCLEOTIDE;
  const uint64_t cap = 1u << 20, W = 4;  // one chunk of the host paths; W words per query cover reads of up to 128 letters
  std::unique_lock<std::mutex> lane_lock(r.lane_mu);
  size_t free_b = 0, total_b = 0;
  const bool hbm_plenty = hipMemGetInfo(&free_b, &total_b) == hipSuccess && free_b > (32ull << 30);
  if (nt) {
    for (int li = 0; li < Replica::NLANES; li++) {  // count_shard_hostpacked
      PackedLane& ln = prepare_count_lane(r, li, cap);
      ln.h_words.ensure(cap * W);
      ensure(ln.words, cap * W);
    }
    for (int li = 0; li < 2; li++) {  // locate_shard_packed
      LocateLane& ln = prepare_locate_lane(r, li, cap, W, 1);
      // hit buffers of a chunk: reads from repeat-rich genomes bring several hits each (7.6 on the GRCh38-shaped text), and a
      // lane whose buffer is too small frees and re-allocates it in the middle of the first call (3-4 ms, four times): room for
      // 16 hits per read (400 MB per lane) while that is a small part of the free HBM, 1.25 otherwise
      static const bool big_hits = !(getenv("AWRY_PREWARM_HITS") && !strcmp(getenv("AWRY_PREWARM_HITS"), "0"));
      const uint64_t hits_cap = hbm_plenty && big_hits ? 16 * cap : cap + cap / 4;
      if (ln.gpos.n < hits_cap) ln.gpos.alloc(hits_cap);
      if (ln.pos.n < 2 * hits_cap) ln.pos.alloc(2 * hits_cap);
    }
    // scratch of the two-phase schedules on the lane streams (survivor lists of a full chunk): for the grids the count plan
    // gives a chunk of 31-mers and a chunk of 101-bp reads (no lists where neither is two-phase on this replica)
    const CountFacts facts = count_facts(r);
    for (int li = 0; li < Replica::NLANES; li++) {
      Replica::SurvScratch* sc = surv_scratch(r, r.lane_stream[li]);
      uint64_t total = 0;
      for (const unsigned nblk : {plan_kmers(facts, cap, 31, true, false).blocks, plan_reads(facts, cap, 101, true, false).blocks})
        if (nblk) total = std::max<uint64_t>(total, list_slots_per_block(cap, nblk) * nblk);
      if (sc->cap < total) { sc->w.alloc(total); sc->range.alloc(total); sc->q.alloc(total); sc->cap = sc->cap_q = total; }
      if (!sc->count.p) sc->count.alloc((size_t)r.num_cus * 8);
      if (!sc->counters.p) sc->counters.alloc(8);
    }
  }
  // pinned result arrays of the locate path (offsets, positions, (record, offset) pairs), taken from the process-wide pool and
  // handed back so that the first call finds them cached.  Pinning is what a first call with large results paid for: 55 ms
  // of a 93 ms awry_locate_batch that returned 735 MB (4 M reads, 30.6 M hits, GRCh38-shaped text) went into ONE growth step
  // of the result arrays, i.e. hipHostMalloc at ~13 GB/s.  AWRY_PINNED_PREWARM_MB (default 1024, capped by the pool's
  // AWRY_PINNED_CACHE_GB) is pinned here instead, as blocks of 64, 64, 128, 256 and 512 MB -- the sizes the arrays of
  // results up to ~750 MB round to; a first call with more than that still pins the excess itself, once.
  static std::once_flag once;
  void* warm_block = nullptr;  // one block stays out until the locate warm-up below has copied into it
  std::call_once(once, [&] {
    const char* e = getenv("AWRY_PINNED_PREWARM_MB");
    const size_t budget = (size_t)((e && atof(e) >= 0 ? atof(e) : 1024.0) * (double)(1u << 20));
    const size_t sizes[5] = {64u << 20, 64u << 20, 128u << 20, 256u << 20, 512u << 20};
    void* blocks[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    size_t used = 0;
    for (int i = 0; i < 5 && used + sizes[i] <= budget; i++) { blocks[i] = PinnedPool::instance().get(sizes[i]); used += sizes[i]; }
    warm_block = blocks[0];
    for (int i = 1; i < 5; i++)
      if (blocks[i]) release_result(blocks[i]);
  });
  // the locate path's own kernels (reads probe with range words, the generic pass over the listed reads, scan, tile/walk/
  // localise) and its copies into pool memory, once per locate lane: 8-9 ms of a first awry_locate_batch were first uses
  // AWRY_PREWARM_LOCATE: bit 0 the reads probe + listed pass, bit 1 scan + locate pass, bit 2 the chunk-sized copies into pool
  // memory (default 7; 0 = none) -- for tools/first_call_ab.sh
  static const int lmask = getenv("AWRY_PREWARM_LOCATE") ? atoi(getenv("AWRY_PREWARM_LOCATE")) : 7;
  const bool warm_locate = lmask != 0;
  if (nt && warm_locate && r.dev.bwt_len >= 4)
    for (int li = 0; li < 2; li++) {
      LocateLane& ln = r.loc_lanes[li];
      hipStream_t s = r.lane_stream[li];
      if (lmask & 1) {
        memset(ln.h_words.p, 0, 16 * W * 8);  // 16 reads of 101 A's: whatever they find, the kernels have run
        HIP_CHECK(hipMemcpyAsync(ln.words.p, ln.h_words.p, 16 * W * 8, hipMemcpyHostToDevice, s));
        HIP_CHECK(hipMemsetAsync(ln.bad.p, 0, 8, s));
        HIP_CHECK(hipMemsetAsync(ln.bad.p + 1, 0xFF, 8, s));
        launch_count_nt2_long(r, ln.words.p, 16, 101, ln.counts.p, ln.rstart.p, true, s, nullptr);
        const QueryList ql{nullptr, nullptr, 0, ln.bad.p, ln.bad.p + 1, 1};  // an empty list: the launch itself is what is warmed
        hipLaunchKernelGGL((count_scalar_kernel<NUCLEOTIDE, LIST_GLOBAL>), dim3(1), dim3(256), 0, s, r.dev, (const uint8_t*)nullptr, (const uint64_t*)nullptr,
                           (uint64_t)0, ln.counts.p, ln.rstart.p, nullptr, 1, (uint64_t)101, ql);
        HIP_CHECK(hipGetLastError());
      }
      if (lmask & 2) {
        // the locate pass on one range that is valid in every index: one hit, the row in the middle of the BWT (RS_PLAIN)
        ln.h_meta.p[0] = r.dev.bwt_len / 2;
        ln.h_meta.p[1] = 1;
        HIP_CHECK(hipMemcpyAsync(ln.rstart.p, ln.h_meta.p, 8, hipMemcpyHostToDevice, s));
        HIP_CHECK(hipMemcpyAsync(ln.counts.p, ln.h_meta.p + 1, 8, hipMemcpyHostToDevice, s));
        launch_scan(r, ln.counts.p, 1, ln.hit_off.p, ln.scratch.p, s);
        launch_locate(r, ln.rstart.p, 1, ln.hit_off.p, 1, 1, ln.gpos.p, ln.pos.p, s);
        HIP_CHECK(hipMemcpyAsync(ln.h_meta.p, ln.hit_off.p + 1, 8, hipMemcpyDeviceToHost, s));
      }
      if (warm_block && (lmask & 4)) {  // chunk-sized copies into pool memory, as the call's results take them
        HIP_CHECK(hipMemcpyAsync(warm_block, ln.gpos.p, cap * 8, hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipMemcpyAsync(static_cast<char*>(warm_block) + cap * 8, ln.pos.p, cap * 16, hipMemcpyDeviceToHost, s));
      }
      HIP_CHECK(hipEventRecord(ln.located, s));
      HIP_CHECK(hipEventSynchronize(ln.located));
      HIP_CHECK(hipStreamSynchronize(s));
    }
  if (warm_block) release_result(warm_block);
  // one round trip per lane stream -- a chunk-sized copy in, the count kernels, a chunk-sized copy out.  Measured: without it the
  // first awry_count_batch of a process spent 17.7 ms enqueueing its first chunks, with a round trip of small copies 7 ms, with
  // chunk-sized ones 0.2 ms (what exactly the runtime sets up on a stream's first use I have not looked at)
  if (nt)
    for (int li = 0; li < Replica::NLANES; li++) {
      PackedLane& ln = r.lanes[li];
      hipStream_t s = r.lane_stream[li];
      memset(ln.h_words.p, 0, cap * 8);  // (a whole chunk each way: large pinned copies take the copy engines, small ones do not)
      const auto c0 = std::chrono::steady_clock::now();
      HIP_CHECK(hipMemcpyAsync(ln.words.p, ln.h_words.p, cap * 8, hipMemcpyHostToDevice, s));
      if (getenv("AWRY_TRACE_HOST"))
        fprintf(stderr, "[awry] warm-up, count lane %d: enqueue of the chunk-sized copy in took %.2f ms\n", li,
                std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - c0).count());
      launch_count_nt2(r, ln.words.p, 64, r.seed_k > 0 && r.seed_k < 31 ? r.seed_k + 1 : 31, ln.counts.p, true, s, nullptr);
      launch_count_nt2_long(r, ln.words.p, 16, 101, ln.counts.p, nullptr, true, s, nullptr);
      hipLaunchKernelGGL(narrow_counts_kernel, dim3(grid_for(r, cap, 1024)), dim3(256), 0, s, ln.counts.p, ln.counts32.p, cap);
      HIP_CHECK(hipMemcpyAsync(ln.h_counts32.p, ln.counts32.p, cap * 4, hipMemcpyDeviceToHost, s));
      HIP_CHECK(hipEventRecord(ln.done, s));
      HIP_CHECK(hipEventSynchronize(ln.done));
      HIP_CHECK(hipStreamSynchronize(s));
    }
  lane_lock.unlock();
  // Last: three chunks of synthetic packed 31-mers through the REAL pipelined count path.  Measured, not explained
  // (tools/first_call_ab.sh, fresh processes on one box, profiles/r03H_first_call_ab.txt): once the warm-up above had run the
  // reads probe with range words (the part that takes 8 ms off the first awry_locate_batch), the first awry_count_batch of the
  // process blocked 11-34 ms inside its first host-to-device copies -- 16 of 19 processes -- although every single operation
  // of that call had been issued here before, and although chunk-sized copies issued here one at a time, in any order and
  // number, returned in 0.01 ms and absorbed nothing.  The stall is paid once, by whichever pipelined call comes first, and
  // never again (count after locate after count: steady).  So the first pipelined call is made here: first awry_count_batch
  // 2.0-2.5 ms against 1.8-2.25 steady in 8 of 8 processes (r03H setting K, r03J setting L), 2.0-4.0 ms in 6 of 6 (r03M); after
  // the chunk copies moved to the replica's copy streams 1.8-2.1 ms in 4 of 5 and 14.9 ms in one (r03d1): it still gets
  // through now and then.  AWRY_PREWARM_REALCOUNT=0 leaves it out (for the A/B).  Tried and dropped: a real-shaped awry_locate_batch of reads without hits as well -- after the count
  // call it left 1 of 5 first count calls at 15 ms again, before it (once or twice) 10 of 16 first locate calls at 13-17 ms
  // where this arrangement gives 7.9-8.6 (profiles/r03J..r03L_first_call_ab.txt).  The first awry_locate_batch therefore
  // still costs ~2.5 ms more than the ones after it (5.5-6.1 ms).
  if (nt && !r.wide && !(getenv("AWRY_PREWARM_REALCOUNT") && !strcmp(getenv("AWRY_PREWARM_REALCOUNT"), "0"))) {
    const uint64_t n = 3ull << 20;
    std::vector<uint64_t> words(n, 0), counts(n, 0);
    PackedPlan plan;
    plan.ok = true;
    plan.Lmax = 31;
    count_shard_hostpacked(r, nullptr, nullptr, Shard{0, n}, plan, counts.data(), words.data());
  }
}

}  // namespace
