// edit_host.h -- the chunk driver of locate within k edits: pigeonhole pieces, their located hits as diagonals, windows, the scan,
// and on request the alignment pass over the hits (awry_align_edit_batch).  Launches, the capacity fallback and the stitching are
// batch_host.h's.
// A part of awry_hip.hip (one translation unit): included there, in order, and not on its own.
#pragma once

namespace {

// ---- locate within k edits (edit_kernels.hip.h) ---------------------------------------------------------------------

static_assert(Q_CANDIDATE_CAP == AWRY_Q_CANDIDATE_CAP && EDIT_MAX_K == AWRY_MAX_EDITS && EDIT_MAX_LEN == AWRY_EDIT_MAX_LEN &&
                  ALIGN_MAX_OPS == AWRY_ALIGN_MAX_OPS,
              "the kernels' limits are the header's");

void require_edits(int k) {
  if (k < 0 || k > EDIT_MAX_K) throw ArgError("max_edits must be in 0..8 (AWRY_MAX_EDITS)");
}

// Candidates (located piece hits) a chunk may hold on the device; a chunk with more, and more than one query, is split in
// halves and each half redone in query order.  Read per call: AWRY_EDIT_CANDIDATE_CAP (tests shrink it).
uint64_t edit_candidate_cap() { return env_cap("AWRY_EDIT_CANDIDATE_CAP", 1ull << 26, 1ull << 31); }

// Hits the alignment pass takes per launch: its fixed-stride staging (text_len, n_ops, ops, and the scan of the run counts: 89 B
// per hit) is bounded by the sub-batch whatever the hit count -- 89 MiB at the default 2^20.  Read per call:
// AWRY_ALIGN_SUB_BATCH (tests shrink it).
uint64_t align_sub_batch() { return env_cap("AWRY_ALIGN_SUB_BATCH", 1ull << 20, 1ull << 24); }

// The text as symbol indices for the scan: the replica's text8 while the verify accelerators keep it, else a copy of the
// replica's own, recovered from the index on first use (one LF chain per file SA sample) and kept with the replica.  Nothing
// else of the replica changes.
const uint8_t* edit_text(Replica& r) {
  if (r.wide || r.dev.bwt_len >= (1ull << 32)) throw ArgError("locate within k edits needs an index with 32-bit rows (bwt_len < 2^32)");
  if (r.dev.text8) return r.dev.text8;
  std::lock_guard<std::mutex> lock(r.edit_mu);
  if (r.edit_text8.p) return r.edit_text8.p;
  DevBuf<uint8_t> t;
  try {
    t.alloc(r.dev.bwt_len + 16);
  } catch (const HipError&) {
    (void)hipGetLastError();
    throw std::bad_alloc();  // AWRY_ERR_OOM
  }
  HIP_CHECK(hipMemsetAsync(t.p, 0, r.dev.bwt_len + 16, r.stream));
  const uint64_t nsamples = (r.dev.bwt_len + r.dev.sa_ratio - 1) / r.dev.sa_ratio;
  with_alphabet(r.dev.alphabet, [&](auto A) {
    hipLaunchKernelGGL(text8_chains_kernel<A()>, dim3(grid_for(r, nsamples, 256, 64)), dim3(256), 0, r.stream, r.dev, nsamples, t.p);
  });
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipStreamSynchronize(r.stream));
  r.edit_text8 = std::move(t);
  return r.edit_text8.p;
}

struct EditHits {  // one shard's result, in query order
  std::vector<uint64_t> counts;  // hits per query
  std::vector<uint8_t> status;   // per query: Q_OK or Q_CANDIDATE_CAP
  std::vector<uint64_t> gpos;
  std::vector<awry_pos_t> pos;
  std::vector<uint8_t> edits;
  std::vector<uint32_t> text_len, cigar;  // the alignment pass: per hit the text span and n_ops runs, the runs back to back
  std::vector<uint8_t> n_ops;
  uint64_t nhits = 0;
};

struct EditWants {  // what the caller asked for: the chunk driver copies back nothing else
  bool pos, gpos, edits, align;
};

// The alignment pass over the nhits hits of a chunk, which lie on the device in window order: their queries out of the windows',
// then per sub-batch the kernel at a fixed stride, a scan of the run counts and the compaction to CSR, appended to `out`.
void align_chunk_hits(Replica& r, const uint8_t* text8, const ChunkBuffers& cb, const uint32_t* win_query, const uint64_t* win_hit_off, uint64_t m,
                      const uint64_t* d_gpos, const uint8_t* d_edits, uint64_t nhits, int k, uint32_t Lmax, EditHits& out) {
  const hipStream_t s = r.stream;
  const uint64_t sub = std::min(align_sub_batch(), nhits);
  DevBuf<uint32_t> hit_query(nhits), text_len(sub), ops(sub * ALIGN_MAX_OPS);
  DevBuf<uint8_t> n_ops(sub);
  DevBuf<uint64_t> counts(sub), cigar_off(sub + 1), scratch(scan_tiles(sub) + 1);
  flat_launch(r, s, nhits, align_hit_query_kernel, win_hit_off, win_query, m, nhits, hit_query.p);
  const size_t at_h = out.text_len.size();
  out.text_len.resize(at_h + nhits);
  out.n_ops.resize(at_h + nhits);
  for (uint64_t at = 0; at < nhits; at += sub) {
    const uint64_t c = std::min(sub, nhits - at);
    launch_edit_align(r, text8, cb.q.p, cb.off.p, hit_query.p + at, d_gpos + at, d_edits + at, c, k, Lmax, text_len.p, n_ops.p, ops.p, s);
    flat_launch(r, s, c, align_counts_kernel, n_ops.p, c, counts.p);
    uint64_t runs = 0;
    scan_with_total(r, counts.p, c, cigar_off.p, scratch.p, &runs, s);
    HIP_CHECK(hipMemcpyAsync(out.text_len.data() + at_h + at, text_len.p, c * 4, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(out.n_ops.data() + at_h + at, n_ops.p, c, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    require(runs <= c * (uint64_t)ALIGN_MAX_OPS, "internal: more CIGAR runs than the bound allows");
    if (runs) {
      DevBuf<uint32_t> cigar(runs);
      flat_launch(r, s, c, align_compact_kernel, ops.p, n_ops.p, cigar_off.p, c, cigar.p);
      const size_t at_c = out.cigar.size();
      out.cigar.resize(at_c + runs);
      HIP_CHECK(hipMemcpyAsync(out.cigar.data() + at_c, cigar.p, runs * 4, hipMemcpyDeviceToHost, s));
      HIP_CHECK(hipStreamSynchronize(s));
    }
  }
}

// One chunk: (1) count the pieces -- the piece CSR is a finer offsets array over the chunk's own bytes -- (2) apply the cap,
// (3) scan and locate the pieces' text positions, (4) diagonals, (5) segmented sort per query, (6) runs of diagonals ->
// windows, (7) scan count pass, (8) scan and fill pass, (9) on request the alignment pass over the hits.  false: the chunk holds
// more candidates than the capacity and more than one query -- nothing appended.
bool edit_chunk(Replica& r, const uint8_t* text8, const uint8_t* qbytes, const uint64_t* qoff, Shard c, int k, uint64_t max_candidates, EditWants want,
                EditHits& out) {
  const bool want_pos = want.pos, want_gpos = want.gpos, want_edits = want.edits;
  const hipStream_t s = r.stream;
  const uint64_t n = c.hi - c.lo, w = (uint64_t)k + 1, np = n * w, n_text = r.dev.bwt_len - 1;
  ChunkBuffers cb;
  upload_chunk(r, cb, qbytes, qoff, c);
  std::vector<uint64_t> h_poff(np + 1);
  uint64_t Lmax = 1;
  for (uint64_t i = 0; i < n; i++) {
    const uint64_t L = cb.h_off[i + 1] - cb.h_off[i];
    if (L == 0) raise_bad_query(c.lo + i, Q_EMPTY);
    if (L > (uint64_t)EDIT_MAX_LEN) throw QueryError("query " + std::to_string(c.lo + i) + ": longer than 256 letters (AWRY_EDIT_MAX_LEN)");
    if (L <= (uint64_t)k) throw QueryError("query " + std::to_string(c.lo + i) + ": not longer than max_edits");
    for (uint64_t t = 0; t < w; t++) h_poff[i * w + t] = cb.h_off[i] + t * L / w;
    Lmax = std::max(Lmax, L);
  }
  h_poff[np] = cb.h_off[n];
  const int W = (int)((Lmax + 63) / 64);
  DevBuf<uint64_t> poff(np + 1), pcounts(np), pranges(2 * np), phoff(np + 1), pscratch(scan_tiles(np) + 1), cand_off(n + 1);
  DevBuf<uint8_t> pstatus(np);
  HIP_CHECK(hipMemcpyAsync(poff.p, h_poff.data(), (np + 1) * 8, hipMemcpyHostToDevice, s));
  launch_count_ascii(r, cb.q.p, poff.p, np, pcounts.p, pranges.p, pstatus.p, s, true);
  flat_launch(r, s, n, edit_cap_kernel, pcounts.p, pstatus.p, n, k, max_candidates, cb.status.p);
  uint64_t total = 0;
  scan_with_total(r, pcounts.p, np, phoff.p, pscratch.p, &total, s);
  HIP_CHECK(hipMemcpyAsync(cb.h_status.data(), cb.status.p, n, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
  for (uint64_t i = 0; i < n; i++)
    if (cb.h_status[i] != Q_OK && cb.h_status[i] != Q_CANDIDATE_CAP) raise_bad_query(c.lo + i, cb.h_status[i]);
  if (total > edit_candidate_cap() && n > 1) return false;
  require(total < (1ull << 32), "one query has 2^32 or more candidates: lower max_candidates");
  std::vector<uint64_t> h_qhoff(n + 1, 0);
  uint64_t m = 0, nhits = 0;
  const size_t at_h = (size_t)out.nhits;
  if (total) {
    DevBuf<uint64_t> cand_gpos(total), key(total), key2(total), heads(total), head_off(total + 1), hscratch(scan_tiles(total) + 1);
    launch_locate(r, pranges.p, 2, phoff.p, np, total, cand_gpos.p, nullptr, s);
    flat_launch(r, s, total, edit_diagonals_kernel, cand_gpos.p, phoff.p, np, total, cb.off.p, k, key.p);
    flat_launch(r, s, n + 1, edit_every_nth_kernel, phoff.p, n + 1, w, cand_off.p);
    unsigned end_bit = 1;
    while (end_bit < 64 && ((r.dev.bwt_len + 2 * (uint64_t)EDIT_MAX_LEN) >> end_bit)) end_bit++;
    size_t tmp_bytes = 0;
    HIP_CHECK(rocprim::segmented_radix_sort_keys(nullptr, tmp_bytes, key.p, key2.p, (unsigned)total, (unsigned)n, cand_off.p, cand_off.p + 1, 0, end_bit, s));
    DevBuf<uint8_t> tmp(std::max<size_t>(tmp_bytes, 8));
    HIP_CHECK(rocprim::segmented_radix_sort_keys(tmp.p, tmp_bytes, key.p, key2.p, (unsigned)total, (unsigned)n, cand_off.p, cand_off.p + 1, 0, end_bit, s));
    flat_launch(r, s, total, edit_run_heads_kernel, key2.p, cand_off.p, n, total, k, heads.p);
    scan_with_total(r, heads.p, total, head_off.p, hscratch.p, &m, s);
    HIP_CHECK(hipStreamSynchronize(s));
    DevBuf<uint32_t> win_query(m), win_count(m);
    DevBuf<uint64_t> run_lo(m), run_hi(m), win_first(m), win_hits(m), win_hit_off(m + 1), wscratch(scan_tiles(m) + 1), q_hit_off(n + 1);
    flat_launch(r, s, total, edit_run_ends_kernel, key2.p, cand_off.p, n, total, k, head_off.p, win_query.p, run_lo.p, run_hi.p);
    flat_launch(r, s, m, edit_windows_kernel, win_query.p, run_lo.p, run_hi.p, m, cb.off.p, k, n_text, win_first.p, win_count.p);
    launch_edit_windows(r, text8, cb.q.p, cb.off.p, win_query.p, win_first.p, win_count.p, m, k, W, n, win_hits.p, nullptr, nullptr, nullptr, s);
    scan_with_total(r, win_hits.p, m, win_hit_off.p, wscratch.p, &nhits, s);
    flat_launch(r, s, n + 1, edit_query_hit_off_kernel, cand_off.p, head_off.p, win_hit_off.p, n, q_hit_off.p);
    HIP_CHECK(hipMemcpyAsync(h_qhoff.data(), q_hit_off.p, (n + 1) * 8, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    if (nhits) {
      DevBuf<uint64_t> d_gpos(nhits), d_pos(want_pos ? 2 * nhits : 0);
      DevBuf<uint8_t> d_edits(nhits);
      launch_edit_windows(r, text8, cb.q.p, cb.off.p, win_query.p, win_first.p, win_count.p, m, k, W, n, nullptr, win_hit_off.p, d_gpos.p, d_edits.p, s);
      if (want_pos) flat_launch(r, s, nhits, edit_localise_kernel, r.dev, nhits, d_gpos.p, d_pos.p);
      if (want_gpos) { out.gpos.resize(at_h + nhits); HIP_CHECK(hipMemcpyAsync(out.gpos.data() + at_h, d_gpos.p, nhits * 8, hipMemcpyDeviceToHost, s)); }
      if (want_pos) { out.pos.resize(at_h + nhits); HIP_CHECK(hipMemcpyAsync(out.pos.data() + at_h, d_pos.p, nhits * 16, hipMemcpyDeviceToHost, s)); }
      if (want_edits) { out.edits.resize(at_h + nhits); HIP_CHECK(hipMemcpyAsync(out.edits.data() + at_h, d_edits.p, nhits, hipMemcpyDeviceToHost, s)); }
      HIP_CHECK(hipStreamSynchronize(s));
      if (want.align) align_chunk_hits(r, text8, cb, win_query.p, win_hit_off.p, m, d_gpos.p, d_edits.p, nhits, k, (uint32_t)Lmax, out);
    }
  }
  require(h_qhoff[n] == nhits, "internal: the queries' hit offsets do not cover the windows'");
  for (uint64_t i = 0; i < n; i++) out.counts.push_back(h_qhoff[i + 1] - h_qhoff[i]);
  out.status.insert(out.status.end(), cb.h_status.begin(), cb.h_status.begin() + n);
  out.nhits += nhits;
  return true;
}

// awry_locate_edit_batch and awry_align_edit_batch (which passes the last three: text_len_out alone, the two cigar arrays together,
// or all): shards over the replicas, results stitched in query order.  The out-pointers are written only when everything has
// succeeded.
void locate_edit_batch(awry_index* idx, const uint8_t* qbytes, const uint64_t* qoff, uint64_t n, int k, uint64_t max_candidates, uint64_t** hit_off_out,
                       awry_pos_t** hits_out, uint64_t** global_pos_out, uint8_t** edits_out, uint8_t** status_out, uint32_t** text_len_out = nullptr,
                       uint64_t** cigar_off_out = nullptr, uint32_t** cigar_out = nullptr) {
  const EditWants want{hits_out != nullptr, global_pos_out != nullptr, edits_out != nullptr, text_len_out != nullptr || cigar_out != nullptr};
  std::vector<EditHits> res(std::max<size_t>(1, idx->reps.size()));
  for_each_replica(idx, n, [&](Replica& r, Shard sh, int g) {
    HIP_CHECK(hipSetDevice(r.device));
    const uint8_t* text8 = edit_text(r);
    for (Shard c : chunk_queries(qoff, sh.lo, sh.hi))
      halve_until_fits(c, [&](Shard h) { return edit_chunk(r, text8, qbytes, qoff, h, k, max_candidates, want, res[g]); });
  });
  MBuf<uint64_t> off, gp, coff;
  MBuf<awry_pos_t> hits;
  MBuf<uint8_t> ed, st;
  MBuf<uint32_t> tl, cg;
  const uint64_t total = stitch_offsets(res, &EditHits::counts, n, off);
  uint64_t nhits = 0;
  for (auto& x : res) {
    if (want.align) require(x.text_len.size() == x.nhits && x.n_ops.size() == x.nhits, "internal: the alignment pass does not cover the hits");
    nhits += x.nhits;
  }
  require(nhits == total, "internal: shard results do not cover the hits");
  if (status_out) stitch_concat(res, &EditHits::status, st);
  if (hits_out) stitch_concat(res, &EditHits::pos, hits);
  if (global_pos_out) stitch_concat(res, &EditHits::gpos, gp);
  if (edits_out) stitch_concat(res, &EditHits::edits, ed);
  if (text_len_out) stitch_concat(res, &EditHits::text_len, tl);
  if (cigar_out) stitch_run_offsets(res, &EditHits::n_ops, total, stitch_concat(res, &EditHits::cigar, cg), coff);
  *hit_off_out = off.release();
  if (hits_out) *hits_out = hits.release();
  if (global_pos_out) *global_pos_out = gp.release();
  if (edits_out) *edits_out = ed.release();
  if (status_out) *status_out = st.release();
  if (text_len_out) *text_len_out = tl.release();
  if (cigar_out) { *cigar_off_out = coff.release(); *cigar_out = cg.release(); }
}

}  // namespace
