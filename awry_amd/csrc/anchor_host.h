// anchor_host.h -- shard drivers of anchors (greedy longest-match factorisation), of SMEMs (all super-maximal exact matches) and
// of locating either: one driver over awry_anchor_t records, parameterised over the launcher that finds them
// A part of awry_hip.hip (one translation unit): included there, in order, and not on its own.
#pragma once

namespace {

// ---- anchors (kernels_anchor.hip.h) and SMEMs (kernels_smem.hip.h) -------------------------------------------------

static_assert(sizeof(Anchor) == sizeof(awry_anchor_t) && sizeof(awry_anchor_t) == 24 && offsetof(Anchor, q_len) == offsetof(awry_anchor_t, q_len) &&
                  offsetof(Anchor, start_row) == offsetof(awry_anchor_t, start_row) && offsetof(Anchor, count) == offsetof(awry_anchor_t, count),
              "the kernels write awry_anchor_t records");

void require_anchor_args(uint32_t min_len, int skip) {
  if (min_len < 1) throw ArgError("min_len must be at least 1");
  if (skip < 0 || skip > 1) throw ArgError("skip must be 0 or 1");
}

// Located hits a chunk may hold on the device; a chunk with more, and more than one query, is split in halves and each half
// redone in query order.  Read per call: AWRY_ANCHOR_HIT_CAP (tests shrink it).
uint64_t anchor_hit_cap() {
  const char* e = getenv("AWRY_ANCHOR_HIT_CAP");
  const uint64_t v = e ? strtoull(e, nullptr, 10) : 0;
  return v ? std::min<uint64_t>(v, 1ull << 31) : (1ull << 26);
}

void require_smem_args(uint32_t min_len) {
  if (min_len < 1) throw ArgError("min_len must be at least 1");
}

// what finds the records: find(r, d_q, d_off, n, d_n, d_rec_off, d_rec, d_status, stream) -- d_rec_off == nullptr is the count
// pass, else the fill pass (launch_anchors' protocol)
auto anchor_finder(uint32_t min_len, int skip) {
  return [=](Replica& r, const uint8_t* d_q, const uint64_t* d_off, uint64_t n, uint64_t* d_n, const uint64_t* d_rec_off, Anchor* d_rec, uint8_t* d_status,
             hipStream_t s) { launch_anchors(r, d_q, d_off, n, min_len, skip, d_n, d_rec_off, d_rec, d_status, s); };
}
auto smem_finder(uint32_t min_len) {
  return [=](Replica& r, const uint8_t* d_q, const uint64_t* d_off, uint64_t n, uint64_t* d_n, const uint64_t* d_rec_off, Anchor* d_rec, uint8_t* d_status,
             hipStream_t s) { launch_smems(r, d_q, d_off, n, min_len, d_n, d_rec_off, d_rec, d_status, s); };
}

struct AnchorHits {  // one shard's result, in query order
  std::vector<uint64_t> n_anchors;     // per query
  std::vector<awry_anchor_t> anchors;
  std::vector<uint64_t> located;       // per anchor: hits located (0 for an anchor of more than max_hits rows)
  std::vector<uint64_t> gpos;
  std::vector<awry_pos_t> pos;
  uint64_t nhits = 0;
};

// count pass, scan, fill pass; with max_hits != 0 also ranges, scan of the located counts and the locate pipeline over the
// flat anchor list.  false: the chunk's located hits exceed the capacity and it holds more than one query -- nothing appended
template <class Find>
bool anchor_chunk(Replica& r, const uint8_t* qbytes, const uint64_t* qoff, Shard c, const Find& find, uint64_t max_hits, bool want_pos, bool want_gpos,
                  AnchorHits& out) {
  const hipStream_t s = r.stream;
  const uint64_t n = c.hi - c.lo;
  for (uint64_t i = c.lo; i < c.hi; i++)
    if (qoff[i + 1] >= qoff[i] && qoff[i + 1] - qoff[i] >= (1ull << 32)) throw ArgError("a query of 2^32 letters or more");
  ChunkBuffers cb;
  upload_chunk(r, cb, qbytes, qoff, c);
  DevBuf<uint64_t> na(n), aoff(n + 1), scratch(scan_tiles(n) + 1);
  find(r, cb.q.p, cb.off.p, n, na.p, nullptr, nullptr, cb.status.p, s);
  launch_scan(r, na.p, n, aoff.p, scratch.p, s);
  uint64_t total = 0;
  HIP_CHECK(hipMemcpyAsync(&total, aoff.p + n, 8, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipMemcpyAsync(cb.h_status.data(), cb.status.p, n, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
  check_status(cb, c.lo);
  if (total >= (1ull << 32)) throw ArgError("a chunk of queries with 2^32 anchors or more");
  DevBuf<Anchor> d_anchors(std::max<uint64_t>(total, 1));
  find(r, cb.q.p, cb.off.p, n, nullptr, aoff.p, d_anchors.p, nullptr, s);
  DevBuf<uint64_t> ranges, located, hoff, lscratch, d_gpos, d_pos;
  uint64_t nhits = 0;
  if (max_hits && total) {
    ranges.alloc(2 * total); located.alloc(total); hoff.alloc(total + 1); lscratch.alloc(scan_tiles(total) + 1);
    launch_anchor_ranges(r, d_anchors.p, total, max_hits, ranges.p, located.p, s);
    launch_scan(r, located.p, total, hoff.p, lscratch.p, s);
    HIP_CHECK(hipMemcpyAsync(&nhits, hoff.p + total, 8, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    if (nhits > anchor_hit_cap() && n > 1) return false;
    if (nhits) {
      d_gpos.alloc(nhits);
      if (want_pos) d_pos.alloc(2 * nhits);
      launch_locate(r, ranges.p, 2, hoff.p, total, nhits, d_gpos.p, d_pos.p, s);
    }
  }
  const size_t at_q = out.n_anchors.size(), at_a = out.anchors.size(), at_h = (size_t)out.nhits;
  out.n_anchors.resize(at_q + n);
  HIP_CHECK(hipMemcpyAsync(out.n_anchors.data() + at_q, na.p, n * 8, hipMemcpyDeviceToHost, s));
  out.anchors.resize(at_a + total);
  if (total) HIP_CHECK(hipMemcpyAsync(out.anchors.data() + at_a, d_anchors.p, total * sizeof(Anchor), hipMemcpyDeviceToHost, s));
  if (max_hits) {
    out.located.resize(at_a + total);
    if (total) HIP_CHECK(hipMemcpyAsync(out.located.data() + at_a, located.p, total * 8, hipMemcpyDeviceToHost, s));
    if (want_gpos) { out.gpos.resize(at_h + nhits); if (nhits) HIP_CHECK(hipMemcpyAsync(out.gpos.data() + at_h, d_gpos.p, nhits * 8, hipMemcpyDeviceToHost, s)); }
    if (want_pos) { out.pos.resize(at_h + nhits); if (nhits) HIP_CHECK(hipMemcpyAsync(out.pos.data() + at_h, d_pos.p, nhits * 16, hipMemcpyDeviceToHost, s)); }
    out.nhits += nhits;
  }
  HIP_CHECK(hipStreamSynchronize(s));
  return true;
}

template <class Find>
void anchor_range(Replica& r, const uint8_t* qbytes, const uint64_t* qoff, Shard c, const Find& find, uint64_t max_hits, bool want_pos, bool want_gpos,
                  AnchorHits& out) {
  if (c.hi <= c.lo) return;
  if (anchor_chunk(r, qbytes, qoff, c, find, max_hits, want_pos, want_gpos, out)) return;
  const uint64_t mid = c.lo + (c.hi - c.lo) / 2;  // the capacity fallback: halves, in query order
  anchor_range(r, qbytes, qoff, Shard{c.lo, mid}, find, max_hits, want_pos, want_gpos, out);
  anchor_range(r, qbytes, qoff, Shard{mid, c.hi}, find, max_hits, want_pos, want_gpos, out);
}

// the batch entry points' common body: shards over the replicas, results stitched in query order into pinned-pool arrays.
// max_hits == 0: records only.  The out-pointers are written only when everything has succeeded.
template <class Find>
void anchor_batch(awry_index* idx, const uint8_t* qbytes, const uint64_t* qoff, uint64_t n, const Find& find, uint64_t max_hits,
                  uint64_t** anchor_off_out, awry_anchor_t** anchors_out, uint64_t** hit_off_out, awry_pos_t** hits_out, uint64_t** global_pos_out) {
  std::vector<AnchorHits> res(std::max<size_t>(1, idx->reps.size()));
  for_each_replica(idx, n, [&](Replica& r, Shard sh, int g) {
    HIP_CHECK(hipSetDevice(r.device));
    for (Shard c : chunk_queries(qoff, sh.lo, sh.hi)) anchor_range(r, qbytes, qoff, c, find, max_hits, hits_out != nullptr, global_pos_out != nullptr, res[g]);
  });
  MBuf<uint64_t> aoff, hoff, gp;
  MBuf<awry_anchor_t> anchors;
  MBuf<awry_pos_t> hits;
  aoff.grow(n + 1);
  aoff.p[0] = 0;
  uint64_t q = 0, total = 0, nhits = 0;
  for (auto& x : res)
    for (uint64_t c : x.n_anchors) { total += c; aoff.p[++q] = total; }
  require(q == n, "internal: shard results do not cover the batch");
  anchors.grow(std::max<uint64_t>(1, total));
  if (max_hits) { hoff.grow(total + 1); hoff.p[0] = 0; }
  uint64_t at = 0;
  for (auto& x : res) {
    if (!x.anchors.empty()) pool_memcpy(anchors.p + at, x.anchors.data(), x.anchors.size() * sizeof(awry_anchor_t));
    if (max_hits)
      for (size_t j = 0; j < x.located.size(); j++) { nhits += x.located[j]; hoff.p[at + j + 1] = nhits; }
    at += x.anchors.size();
  }
  require(at == total, "internal: shard results do not cover the anchors");
  if (hits_out) hits.grow(std::max<uint64_t>(1, nhits));
  if (global_pos_out) gp.grow(std::max<uint64_t>(1, nhits));
  uint64_t ath = 0;
  for (auto& x : res) {
    if (hits_out && x.nhits) pool_memcpy(hits.p + ath, x.pos.data(), x.nhits * sizeof(awry_pos_t));
    if (global_pos_out && x.nhits) pool_memcpy(gp.p + ath, x.gpos.data(), x.nhits * 8);
    ath += x.nhits;
  }
  *anchor_off_out = aoff.release();
  *anchors_out = anchors.release();
  if (hit_off_out) *hit_off_out = hoff.release();
  if (hits_out) *hits_out = hits.release();
  if (global_pos_out) *global_pos_out = gp.release();
}

}  // namespace
