// anchor_host.h -- shard drivers of anchors (greedy longest-match factorisation), of SMEMs (all super-maximal exact matches) and
// of locating either: one driver over awry_anchor_t records, parameterised over the launcher that finds them.  Its device part,
// the record-locate stage (find_records, locate_records), is also the first stage of chain_chunk (chain_host.h).
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
uint64_t anchor_hit_cap() { return env_cap("AWRY_ANCHOR_HIT_CAP", 1ull << 26, 1ull << 31); }

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

// ---- the record-locate stage: shared by anchor_chunk, which copies its results out, and chain_chunk (chain_host.h), which goes
// on to seeds on the device --------------------------------------------------------------------------------------------------------

struct LocatedRecords {  // what the stage leaves on the device
  ChunkBuffers cb, up;                         // the chunk's queries; `up` holds the reads as given when every read is two queries
  DevBuf<uint64_t> n_rec, rec_off, scratch;    // per query: records, their offsets; the scratch of scans over the queries
  DevBuf<Anchor> rec;                          // the `total` records
  DevBuf<uint64_t> ranges, located, hit_off, lscratch;  // per record: rows, hits located (0 over max_hits), their offsets
  DevBuf<uint64_t> gpos, pos;                  // the `nhits` located hits: text positions, and on request (record, offset) pairs
  uint64_t total = 0, nhits = 0;
  void release_records() { rec.reset(); ranges.reset(); located.reset(); hit_off.reset(); lscratch.reset(); }
};

// Upload, count pass, scan, status check, fill pass; with max_hits != 0 also the records' ranges and the scan of the located
// counts.  copies == 2: the reads are uploaded once and expanded on the device into the doubled batch (launch_strand_expand: query
// 2i = read i, query 2i + 1 = its reverse complement); everything after that is over the 2 (c.hi - c.lo) queries, a rejected query
// is raised under its read's index, and the capacity test counts reads, so a read's two strands are never split.  `what` names the
// records in the message of a chunk with 2^32 of them.  false: the chunk's located hits exceed the capacity and it holds more than
// one read -- nothing has been located.  Two stream synchronisations (one with max_hits == 0 or without records).  unit: the reads
// that are never split (2: a read pair) -- a chunk of one unit is never refused, or its halving would not end.
template <class Find>
bool find_records(Replica& r, const uint8_t* qbytes, const uint64_t* qoff, Shard c, const Find& find, uint64_t max_hits, int copies, const char* what,
                  LocatedRecords& L, uint64_t unit = 1) {
  const hipStream_t s = r.stream;
  const uint64_t nreads = c.hi - c.lo, n = copies * nreads;
  ChunkBuffers& cb = L.cb;
  upload_chunk(r, copies == 2 ? L.up : cb, qbytes, qoff, c);
  if (copies == 2) {
    const ChunkBuffers& up = L.up;
    const uint64_t nbytes = up.h_off[nreads];
    cb.q.alloc(2 * nbytes + 16);
    cb.off.alloc(n + 1);
    cb.status.alloc(std::max<uint64_t>(n, 1));
    cb.h_off.resize(n + 1);
    for (uint64_t i = 0; i < nreads; i++) {
      cb.h_off[2 * i] = 2 * up.h_off[i];
      cb.h_off[2 * i + 1] = 2 * up.h_off[i] + (up.h_off[i + 1] - up.h_off[i]);
    }
    cb.h_off[n] = 2 * nbytes;
    cb.h_status.resize(n);
    launch_strand_expand(r, up.q.p, up.off.p, nreads, cb.q.p, cb.off.p, s);
  }
  L.n_rec.alloc(n); L.rec_off.alloc(n + 1); L.scratch.alloc(scan_tiles(n) + 1);
  find(r, cb.q.p, cb.off.p, n, L.n_rec.p, nullptr, nullptr, cb.status.p, s);
  scan_with_total(r, L.n_rec.p, n, L.rec_off.p, L.scratch.p, &L.total, s);
  HIP_CHECK(hipMemcpyAsync(cb.h_status.data(), cb.status.p, n, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
  for (uint64_t i = 0; i < n; i++)
    if (cb.h_status[i] != Q_OK) raise_bad_query(c.lo + i / copies, cb.h_status[i]);  // the read's own index
  const uint64_t total = L.total;
  if (total >= (1ull << 32)) throw ArgError(std::string("a chunk of queries with 2^32 ") + what + " or more");
  if (!total) return true;
  L.rec.alloc(total);
  if (max_hits) { L.ranges.alloc(2 * total); L.located.alloc(total); L.hit_off.alloc(total + 1); L.lscratch.alloc(scan_tiles(total) + 1); }
  find(r, cb.q.p, cb.off.p, n, nullptr, L.rec_off.p, L.rec.p, nullptr, s);
  if (!max_hits) return true;
  launch_anchor_ranges(r, L.rec.p, total, max_hits, L.ranges.p, L.located.p, s);
  scan_with_total(r, L.located.p, total, L.hit_off.p, L.lscratch.p, &L.nhits, s);
  HIP_CHECK(hipStreamSynchronize(s));
  return !(L.nhits > anchor_hit_cap() && nreads > unit);
}

// the locate pipeline over the flat record list: text positions, and with want_pos (record, offset) pairs
void locate_records(Replica& r, LocatedRecords& L, bool want_pos) {
  if (!L.nhits) return;
  L.gpos.alloc(L.nhits);
  if (want_pos) L.pos.alloc(2 * L.nhits);
  launch_locate(r, L.ranges.p, 2, L.hit_off.p, L.total, L.nhits, L.gpos.p, L.pos.p, r.stream);
}

// the stage with max_hits != 0, or the records alone; then the copy-out.  false: over capacity (find_records) -- nothing appended
template <class Find>
bool anchor_chunk(Replica& r, const uint8_t* qbytes, const uint64_t* qoff, Shard c, const Find& find, uint64_t max_hits, bool want_pos, bool want_gpos,
                  AnchorHits& out) {
  const hipStream_t s = r.stream;
  const uint64_t n = c.hi - c.lo;
  for (uint64_t i = c.lo; i < c.hi; i++)
    if (qoff[i + 1] >= qoff[i] && qoff[i + 1] - qoff[i] >= (1ull << 32)) throw ArgError("a query of 2^32 letters or more");
  LocatedRecords L;
  if (!find_records(r, qbytes, qoff, c, find, max_hits, 1, "anchors", L)) return false;
  locate_records(r, L, want_pos);
  const uint64_t total = L.total, nhits = L.nhits;
  const size_t at_q = out.n_anchors.size(), at_a = out.anchors.size(), at_h = (size_t)out.nhits;
  out.n_anchors.resize(at_q + n);
  HIP_CHECK(hipMemcpyAsync(out.n_anchors.data() + at_q, L.n_rec.p, n * 8, hipMemcpyDeviceToHost, s));
  out.anchors.resize(at_a + total);
  if (total) HIP_CHECK(hipMemcpyAsync(out.anchors.data() + at_a, L.rec.p, total * sizeof(Anchor), hipMemcpyDeviceToHost, s));
  if (max_hits) {
    out.located.resize(at_a + total);
    if (total) HIP_CHECK(hipMemcpyAsync(out.located.data() + at_a, L.located.p, total * 8, hipMemcpyDeviceToHost, s));
    if (want_gpos) { out.gpos.resize(at_h + nhits); if (nhits) HIP_CHECK(hipMemcpyAsync(out.gpos.data() + at_h, L.gpos.p, nhits * 8, hipMemcpyDeviceToHost, s)); }
    if (want_pos) { out.pos.resize(at_h + nhits); if (nhits) HIP_CHECK(hipMemcpyAsync(out.pos.data() + at_h, L.pos.p, nhits * 16, hipMemcpyDeviceToHost, s)); }
    out.nhits += nhits;
  }
  HIP_CHECK(hipStreamSynchronize(s));
  return true;
}

// the batch entry points' common body: shards over the replicas, results stitched in query order into pinned-pool arrays.
// max_hits == 0: records only.  The out-pointers are written only when everything has succeeded.
template <class Find>
void anchor_batch(awry_index* idx, const uint8_t* qbytes, const uint64_t* qoff, uint64_t n, const Find& find, uint64_t max_hits,
                  uint64_t** anchor_off_out, awry_anchor_t** anchors_out, uint64_t** hit_off_out, awry_pos_t** hits_out, uint64_t** global_pos_out) {
  std::vector<AnchorHits> res(std::max<size_t>(1, idx->reps.size()));
  for_each_replica(idx, n, [&](Replica& r, Shard sh, int g) {
    HIP_CHECK(hipSetDevice(r.device));
    for (Shard c : chunk_queries(qoff, sh.lo, sh.hi))
      halve_until_fits(c, [&](Shard h) { return anchor_chunk(r, qbytes, qoff, h, find, max_hits, hits_out != nullptr, global_pos_out != nullptr, res[g]); });
  });
  MBuf<uint64_t> aoff, hoff, gp;
  MBuf<awry_anchor_t> anchors;
  MBuf<awry_pos_t> hits;
  const uint64_t total = stitch_offsets(res, &AnchorHits::n_anchors, n, aoff);
  require(stitch_concat(res, &AnchorHits::anchors, anchors) == total, "internal: shard results do not cover the anchors");
  if (max_hits) {  // the located counts are per anchor: their offsets run over the whole batch's anchors
    hoff.grow(total + 1);
    hoff.p[0] = 0;
    uint64_t at = 0, nhits = 0;
    for (auto& x : res)
      for (uint64_t c : x.located) { require(at < total, "internal: shard results do not cover the anchors"); nhits += c; hoff.p[++at] = nhits; }
    require(at == total, "internal: shard results do not cover the anchors");
  }
  if (hits_out) stitch_concat(res, &AnchorHits::pos, hits);
  if (global_pos_out) stitch_concat(res, &AnchorHits::gpos, gp);
  *anchor_off_out = aoff.release();
  *anchors_out = anchors.release();
  if (hit_off_out) *hit_off_out = hoff.release();
  if (hits_out) *hits_out = hits.release();
  if (global_pos_out) *global_pos_out = gp.release();
}

}  // namespace
