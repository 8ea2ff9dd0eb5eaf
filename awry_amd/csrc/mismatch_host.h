// mismatch_host.h -- shard drivers of the substitution-tolerant and class-pattern count and locate (launches, the capacity
// fallback and the stitching are batch_host.h's)
// A part of awry_hip.hip (one translation unit): included there, in order, and not on its own.
#pragma once

namespace {

// ---- substitution-tolerant and class-pattern count / locate (mismatch_kernels.hip.h) ----------------------
// `classes` selects the kernel's mode (launch_count_leaves); everything after the leaves is shared: chunking, the leaf cap,
// segmented sort by first row, launch_locate, per-hit distance.  Queries are validated where they are searched (lane refill
// of the kernel), and a rejected or abandoned one fails the batch through its status byte, before any result array is handed out.

static_assert(PT_MAX_CLASS == AWRY_MAX_CLASS_POSITIONS && PT_MAX_FRAMES == AWRY_PATTERN_MAX_FRAMES && MM_MAX_K == AWRY_MAX_MISMATCHES,
              "the kernel's limits are the header's");
static_assert(Q_NOT_CLASS_LETTER == AWRY_Q_NOT_CLASS_LETTER && Q_CLASS_POSITIONS == AWRY_Q_CLASS_POSITIONS && Q_EXPANSION_CAP == AWRY_Q_EXPANSION_CAP,
              "the kernel's status bytes are the header's");

void require_mismatches(int k) {
  if (k < 0 || k > MM_MAX_K) throw ArgError("max_mismatches must be 0, 1 or 2");
}

void count_mismatch_shard(Replica& r, const uint8_t* qbytes, const uint64_t* qoff, Shard sh, int k, uint64_t* counts_out, bool classes) {
  HIP_CHECK(hipSetDevice(r.device));
  ChunkBuffers cb;
  for (Shard c : chunk_queries(qoff, sh.lo, sh.hi)) {
    const uint64_t n = c.hi - c.lo, w = (uint64_t)(k + 1);
    upload_chunk(r, cb, qbytes, qoff, c);
    if (cb.counts.n < n * w) cb.counts.alloc(n * w);
    launch_count_leaves(r, classes, cb.q.p, cb.off.p, n, k, cb.counts.p, nullptr, nullptr, cb.status.p, r.stream, nullptr, nullptr, nullptr, nullptr);
    HIP_CHECK(hipMemcpyAsync(cb.h_status.data(), cb.status.p, n, hipMemcpyDeviceToHost, r.stream));
    HIP_CHECK(hipMemcpyAsync(counts_out + c.lo * w, cb.counts.p, n * w * 8, hipMemcpyDeviceToHost, r.stream));
    HIP_CHECK(hipStreamSynchronize(r.stream));
    check_status(cb, c.lo);
  }
}

// Leaves (row ranges of the variants that occur) a locate chunk may hold on the device; a chunk with more is split in halves
// and each half redone (one query with more gets what it needs).  Read per call: AWRY_MISMATCH_LEAF_CAP (tests shrink it).
uint64_t mismatch_leaf_cap() { return env_cap("AWRY_MISMATCH_LEAF_CAP", 1ull << 26, 1ull << 31); }

struct MismatchHits {  // one shard's locate result, in query order
  std::vector<uint64_t> counts;  // hits per query
  std::vector<uint64_t> gpos;
  std::vector<awry_pos_t> pos;
  std::vector<uint8_t> mm;
};

// pass 1 (counts, leaves per query), scans, pass 2 (leaves), segmented sort by first row within each query, locate over the
// flat leaf list, distances per hit.  false: the chunk holds more leaves than the cap and more than one query -- nothing appended
bool locate_mismatch_chunk(Replica& r, const uint8_t* qbytes, const uint64_t* qoff, Shard c, int k, bool want_pos, bool want_gpos, bool want_mm,
                           MismatchHits& out, bool classes) {
  const hipStream_t s = r.stream;
  const uint64_t n = c.hi - c.lo;
  ChunkBuffers cb;
  upload_chunk(r, cb, qbytes, qoff, c);
  DevBuf<uint64_t> totals(n), nleaves(n), hit_off(n + 1), leaf_off(n + 1), scratch(scan_tiles(n) + 1);
  launch_count_leaves(r, classes, cb.q.p, cb.off.p, n, k, nullptr, totals.p, nleaves.p, cb.status.p, s, nullptr, nullptr, nullptr, nullptr);
  uint64_t total = 0, nleaf = 0;
  scan_with_total(r, totals.p, n, hit_off.p, scratch.p, &total, s);
  scan_with_total(r, nleaves.p, n, leaf_off.p, scratch.p, &nleaf, s);
  HIP_CHECK(hipMemcpyAsync(cb.h_status.data(), cb.status.p, n, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
  check_status(cb, c.lo);
  if (nleaf > mismatch_leaf_cap() && n > 1) return false;
  require(nleaf < (1ull << 32), "one query has 2^32 or more occurring variants");
  const size_t at_q = out.counts.size(), at_h = out.gpos.size();
  out.counts.resize(at_q + n);
  HIP_CHECK(hipMemcpyAsync(out.counts.data() + at_q, totals.p, n * 8, hipMemcpyDeviceToHost, s));
  if (total) {
    DevBuf<uint64_t> key(nleaf), val(nleaf), key2(nleaf), val2(nleaf), width(nleaf), leaf_hit_off(nleaf + 1), lscratch(scan_tiles(nleaf) + 1);
    launch_count_leaves(r, classes, cb.q.p, cb.off.p, n, k, nullptr, nullptr, nullptr, nullptr, s, nullptr, leaf_off.p, key.p, val.p);
    // DFS from the right end does not visit the leaves in row order: sort each query's leaves by their first row
    unsigned end_bit = 1;
    while (end_bit < 64 && (r.dev.bwt_len >> end_bit)) end_bit++;
    size_t tmp_bytes = 0;
    HIP_CHECK(rocprim::segmented_radix_sort_pairs(nullptr, tmp_bytes, key.p, key2.p, val.p, val2.p, (unsigned)nleaf, (unsigned)n, leaf_off.p,
                                                  leaf_off.p + 1, 0, end_bit, s));
    DevBuf<uint8_t> tmp(std::max<size_t>(tmp_bytes, 8));
    HIP_CHECK(rocprim::segmented_radix_sort_pairs(tmp.p, tmp_bytes, key.p, key2.p, val.p, val2.p, (unsigned)nleaf, (unsigned)n, leaf_off.p,
                                                  leaf_off.p + 1, 0, end_bit, s));
    flat_launch(r, s, nleaf, mm_leaf_widths_kernel, val2.p, nleaf, width.p);
    launch_scan(r, width.p, nleaf, leaf_hit_off.p, lscratch.p, s);
    DevBuf<uint64_t> d_gpos(total), d_pos(want_pos ? 2 * total : 0);
    DevBuf<uint8_t> d_mm(want_mm ? total : 0);
    launch_locate(r, key2.p, 1, leaf_hit_off.p, nleaf, total, d_gpos.p, d_pos.p, s);
    if (want_mm) flat_launch(r, s, total, mm_hit_distance_kernel, leaf_hit_off.p, val2.p, nleaf, total, d_mm.p);
    if (want_gpos) { out.gpos.resize(at_h + total); HIP_CHECK(hipMemcpyAsync(out.gpos.data() + at_h, d_gpos.p, total * 8, hipMemcpyDeviceToHost, s)); }
    if (want_pos) { out.pos.resize(at_h + total); HIP_CHECK(hipMemcpyAsync(out.pos.data() + at_h, d_pos.p, total * 16, hipMemcpyDeviceToHost, s)); }
    if (want_mm) { out.mm.resize(at_h + total); HIP_CHECK(hipMemcpyAsync(out.mm.data() + at_h, d_mm.p, total, hipMemcpyDeviceToHost, s)); }
  }
  HIP_CHECK(hipStreamSynchronize(s));
  return true;
}

// the host batch drivers of both modes (awry_count_mismatch_batch / awry_count_pattern_batch, and the locate pair)
void count_leaves_batch(awry_index* idx, const uint8_t* qbytes, const uint64_t* qoff, uint64_t n, int k, uint64_t* counts_out, bool classes) {
  require(idx && qoff && (counts_out || n == 0), "null argument");
  require(qbytes || qoff[n] == qoff[0], "null query bytes");
  require_mismatches(k);
  for_each_replica(idx, n, [&](Replica& r, Shard sh, int) { count_mismatch_shard(r, qbytes, qoff, sh, k, counts_out, classes); });
}

void locate_leaves_batch(awry_index* idx, const uint8_t* qbytes, const uint64_t* qoff, uint64_t n, int k, uint64_t** hit_off_out,
                         awry_pos_t** hits_out, uint64_t** global_pos_out, uint8_t** mismatches_out, bool classes) {
  require(idx && qoff && hit_off_out, "null argument");
  require(qbytes || qoff[n] == qoff[0], "null query bytes");
  require_mismatches(k);
  std::vector<MismatchHits> res(std::max<size_t>(1, idx->reps.size()));
  for_each_replica(idx, n, [&](Replica& r, Shard sh, int g) {
    HIP_CHECK(hipSetDevice(r.device));
    const bool want_pos = hits_out != nullptr, want_gpos = global_pos_out != nullptr, want_mm = mismatches_out != nullptr;
    for (Shard c : chunk_queries(qoff, sh.lo, sh.hi))
      halve_until_fits(c, [&](Shard h) { return locate_mismatch_chunk(r, qbytes, qoff, h, k, want_pos, want_gpos, want_mm, res[g], classes); });
  });
  MBuf<uint64_t> off, gp;
  MBuf<awry_pos_t> hits;
  MBuf<uint8_t> mm;
  stitch_offsets(res, &MismatchHits::counts, n, off);
  if (hits_out) stitch_concat(res, &MismatchHits::pos, hits);
  if (global_pos_out) stitch_concat(res, &MismatchHits::gpos, gp);
  if (mismatches_out) stitch_concat(res, &MismatchHits::mm, mm);
  *hit_off_out = off.release();
  if (hits_out) *hits_out = hits.release();
  if (global_pos_out) *global_pos_out = gp.release();
  if (mismatches_out) *mismatches_out = mm.release();
}

// the device-resident count of both modes (awry_dev_count_mismatch_tally / awry_dev_count_pattern_tally)
void dev_count_leaves(awry_index* idx, int slot, bool classes, const void* d_qbytes, const void* d_qoff, uint64_t n, int k, void* d_counts,
                      void* d_status, void* d_tally, void* stream) {
  require_mismatches(k);
  Replica& r = replica(idx, slot);
  require(n == 0 || (d_qbytes && d_qoff && d_counts), "null argument");
  launch_count_leaves(r, classes, (const uint8_t*)d_qbytes, (const uint64_t*)d_qoff, n, k, (uint64_t*)d_counts, nullptr, nullptr, (uint8_t*)d_status,
                      (hipStream_t)stream, (unsigned long long*)d_tally);
}

}  // namespace
