// pair_host.h -- the driver of awry_map_pairs_batch, a sink of chain_chunk over the doubled batch of 2 P reads (chain_host.h, both
// strands), after map_chunk (map_host.h): the kept lists of every read (map_select at max_report = 2 A), the rescue windows, the edit
// scan over them and the aligner over each window's best hit (edit_host.h's launchers), the rescued candidates, the pair choice
// (count pass, scan, fill pass), and the CIGARs of the chosen records: chain-derived ones through fill_reported_cigars, rescued ones
// out of the aligner's fixed-stride runs.
// A part of awry_hip.hip (one translation unit): included there, in order, after map_host.h, and not on its own.
#pragma once

namespace {

// ---- map read pairs (kernels_pair.hip.h) --------------------------------------------------------------------------------------

static_assert(PAIR_MAX_INSERT == AWRY_PAIR_MAX_INSERT && PAIR_MAX_ANCHORS == AWRY_PAIR_MAX_ANCHORS && PAIR_NO_CHAIN == AWRY_PAIR_NO_CHAIN &&
                  MAP_PROPER_PAIR == AWRY_MAP_PROPER_PAIR && MAP_RESCUED == AWRY_MAP_RESCUED && MAP_MATE_UNMAPPED == AWRY_MAP_MATE_UNMAPPED,
              "the kernels' limits and flags are the header's");

static_assert(PAIR_CLIP_MAX_UNPAIRED == AWRY_PAIR_CLIP_MAX_UNPAIRED && PAIR_CLIP_MAX_UNPAIRED == CHAIN_ALIGN_MAX_LEN * AWRY_CLIP_MAX_MATCH,
              "the clipped mode's penalty bound is the header's: the largest score of a read");

// clipped = false: unpaired_penalty in edits; true: in score units
PairParams pair_params(uint64_t min_insert, uint64_t max_insert, uint32_t unpaired_penalty, uint32_t rescue_anchors, int rescue_edits, bool clipped = false) {
  if (max_insert > (uint64_t)PAIR_MAX_INSERT) throw ArgError("max_insert must be at most 2^20 (AWRY_PAIR_MAX_INSERT)");
  if (min_insert > max_insert) throw ArgError("min_insert must not exceed max_insert");
  if (!clipped && unpaired_penalty > 255) throw ArgError("unpaired_penalty must be in 0..255");
  if (clipped && unpaired_penalty > PAIR_CLIP_MAX_UNPAIRED) throw ArgError("unpaired_penalty must be in 0..16384 (AWRY_PAIR_CLIP_MAX_UNPAIRED)");
  if (rescue_anchors > (uint32_t)PAIR_MAX_ANCHORS) throw ArgError("rescue_anchors must be in 0..4 (AWRY_PAIR_MAX_ANCHORS)");
  if (rescue_edits < 0 || rescue_edits > EDIT_MAX_K) throw ArgError("rescue_edits must be in 0..8 (AWRY_MAX_EDITS)");
  return PairParams{(uint32_t)min_insert, (uint32_t)max_insert, unpaired_penalty, rescue_anchors, (uint32_t)rescue_edits};
}

// Starts a rescue window hands to one lane of the edit scan: longer windows are cut (the hit rule does not see the cut).  Read per
// call: AWRY_PAIR_SUB_WINDOW (tests change it).
uint32_t pair_sub_window() { return (uint32_t)env_cap("AWRY_PAIR_SUB_WINDOW", 64, 1ull << 21); }

// the clipped pair choice's mode: the weights of a rescued candidate's score, the threshold T and the MAPQ divisor a + b
PairMode clip_pair_mode(const AlignMode& md, const MapMode& mm) { return PairMode{true, md.match, md.mismatch, md.gap, mm.min_score, mm.mapq_div}; }

template <class MapT>  // awry_map_t, or awry_map_clip_t in the clipped mode
struct PairHitsOf {  // one shard's result, in read order (insert: in pair order)
  std::vector<uint64_t> n_maps;  // per read: 0 or 1
  std::vector<uint8_t> status;   // per read: Q_OK or Q_SEED_CAP
  std::vector<MapT> maps;
  std::vector<awry_pos_t> pos;
  std::vector<uint64_t> n_ops;  // per record
  std::vector<uint32_t> cigar;  // the runs, back to back
  std::vector<uint32_t> insert;
};

// One chunk of whole pairs, from where chain_chunk's fill pass leaves the doubled batch (4 queries a pair): steps 1 - 3 are
// map_chunk's with max_report = 2 A, so that every kept candidate of a read is a record on the device.  MapT is the record of the
// mode: md for the alignment, mm for the kept lists, pm for the rescued candidates and the pair choice.
template <class MapT>
void pair_chunk(Replica& r, const uint8_t* text8, const ChainOnDevice& v, uint32_t A, int band, const AlignMode& md, const MapMode& mm, const PairMode& pm,
                const PairParams& pp, bool want_pos, bool want_cigar, PairHitsOf<MapT>& out) {
  constexpr bool CLIP = std::is_same_v<MapT, awry_map_clip_t>;
  using Rec = MapRecOf<CLIP>;
  require(md.clip == CLIP && mm.clip == CLIP && pm.clip == CLIP, "internal: the pair records are not the mode's");
  const hipStream_t s = r.stream;
  const uint64_t n = v.c.hi - v.c.lo, n2 = 2 * n, P = n / 2;
  const int k = (int)pp.rescue_edits;
  require(n % 2 == 0, "internal: a chunk of read pairs holds an odd number of reads");
  uint64_t Lmax = 1, Lresc = 0;  // the longest read, and the longest one the edit scan takes
  for (uint64_t i = 0; i < n2; i += 2) {
    const uint64_t L = v.cb.h_off[i + 1] - v.cb.h_off[i];
    Lmax = std::max(Lmax, L);
    if (L <= (uint64_t)EDIT_MAX_LEN) Lresc = std::max(Lresc, L);
  }
  SelectedChains S;
  select_chains(r, v, n2, (uint64_t)A, S);
  const uint64_t total = S.total;
  if (!total) { S.query.alloc(1); S.chains.alloc(1); S.moff.alloc(1); }
  DevBuf<uint64_t> nops(std::max<uint64_t>(total, 1));
  DevBuf<AlnOf<CLIP>> alns(std::max<uint64_t>(total, 1));
  if (total) {
    const uint64_t sub = std::min(chain_align_sub_batch(), total);
    for (uint64_t at = 0; at < total; at += sub)
      launch_chain_align(r, text8, v.cb.q.p, v.cb.off.p, S.query.p + at, S.moff.p + at, S.members.p, std::min(sub, total - at), band, md,
                         (uint32_t)Lmax, alns.p + at, nops.p + at, nullptr, nullptr, s);
    S.release_scratch();
  }
  // the kept lists: every read's candidates in rank order, and per candidate the index of its alignment
  DevBuf<uint64_t> nkept(n), koff(n + 1);
  DevBuf<uint8_t> rstatus(n);
  launch_map_select(r, S.aoff.p, alns.p, S.chains.p, v.status, n, A, 2 * A, mm, nkept.p, rstatus.p, nullptr, nullptr, nullptr, nullptr, s);
  launch_scan(r, nkept.p, n, koff.p, S.scratch.p, s);
  uint64_t ncand = 0;
  const size_t at_q = out.n_maps.size(), at_m = out.maps.size(), at_p = out.insert.size();
  out.n_maps.resize(at_q + n);
  out.status.resize(at_q + n);
  out.insert.resize(at_p + P);  // (zeros: what a chunk without a record reports)
  HIP_CHECK(hipMemcpyAsync(&ncand, koff.p + n, 8, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipMemcpyAsync(out.status.data() + at_q, rstatus.p, n, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
  require(ncand <= total, "internal: more candidates kept than aligned");
  if (!ncand) return;  // (n_maps stays zero)
  DevBuf<Rec> cands(ncand);
  DevBuf<uint32_t> cand_aln(ncand);
  launch_map_select(r, S.aoff.p, alns.p, S.chains.p, v.status, n, A, 2 * A, mm, nullptr, nullptr, koff.p, cands.p, cand_aln.p, nullptr, s);
  // mate rescue: windows, cut for the scan; the scan's count pass, scan, fill pass; the best hit of each window; its alignment
  const uint64_t slots = n * pp.rescue_anchors;
  DevBuf<Rec> resc;
  DevBuf<uint32_t> win_query, win_count, sub_query, sub_count, text_len, r_ops;
  DevBuf<uint64_t> win_first, n_sub, sub_off, sscratch, sub_first, n_hits, hit_off, hscratch, hit_gpos, best_gpos;
  DevBuf<uint8_t> hit_edits, best_edits, r_nops;
  if (slots && Lresc > (uint64_t)k) {
    win_query.alloc(slots); win_count.alloc(slots); win_first.alloc(slots);
    n_sub.alloc(slots); sub_off.alloc(slots + 1); sscratch.alloc(scan_tiles(slots) + 1);
    launch_pair_windows(r, koff.p, cands.p, v.cb.off.p, 2, P, pp, win_query.p, win_first.p, win_count.p, s);
    const uint32_t sub = pair_sub_window();
    flat_launch(r, s, slots, pair_sub_windows_kernel<false>, win_query.p, win_first.p, win_count.p, slots, sub, n_sub.p, nullptr, nullptr, nullptr, nullptr);
    launch_scan(r, n_sub.p, slots, sub_off.p, sscratch.p, s);
    uint64_t m = 0, nhits = 0;
    HIP_CHECK(hipMemcpyAsync(&m, sub_off.p + slots, 8, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    if (m) {
      sub_query.alloc(m); sub_count.alloc(m); sub_first.alloc(m); n_hits.alloc(m); hit_off.alloc(m + 1); hscratch.alloc(scan_tiles(m) + 1);
      flat_launch(r, s, slots, pair_sub_windows_kernel<true>, win_query.p, win_first.p, win_count.p, slots, sub, nullptr, sub_off.p, sub_query.p, sub_first.p,
                  sub_count.p);
      // the masks per query of the doubled batch, at the words the longest rescuable read needs: a longer read has no window, and
      // the scan takes no query of more than 64 W letters
      const int W = (int)((Lresc + 63) / 64);
      launch_edit_windows(r, text8, v.cb.q.p, v.cb.off.p, sub_query.p, sub_first.p, sub_count.p, m, k, W, n2, n_hits.p, nullptr, nullptr, nullptr, s);
      launch_scan(r, n_hits.p, m, hit_off.p, hscratch.p, s);
      HIP_CHECK(hipMemcpyAsync(&nhits, hit_off.p + m, 8, hipMemcpyDeviceToHost, s));
      HIP_CHECK(hipStreamSynchronize(s));
    }
    if (nhits) {
      hit_gpos.alloc(nhits); hit_edits.alloc(nhits); best_gpos.alloc(slots); best_edits.alloc(slots);
      text_len.alloc(slots); r_nops.alloc(slots); r_ops.alloc(slots * ALIGN_MAX_OPS); resc.alloc(slots);
      const int W = (int)((Lresc + 63) / 64);
      launch_edit_windows(r, text8, v.cb.q.p, v.cb.off.p, sub_query.p, sub_first.p, sub_count.p, m, k, W, n2, nullptr, hit_off.p, hit_gpos.p, hit_edits.p, s);
      flat_launch(r, s, slots, pair_best_hit_kernel, sub_off.p, hit_off.p, hit_gpos.p, hit_edits.p, slots, best_gpos.p, best_edits.p);
      launch_edit_align(r, text8, v.cb.q.p, v.cb.off.p, win_query.p, best_gpos.p, best_edits.p, slots, k, (uint32_t)Lresc, text_len.p, r_nops.p, r_ops.p, s);
      flat_launch(r, s, slots, pair_rescued_kernel<Rec>, win_query.p, best_gpos.p, best_edits.p, text_len.p, r_nops.p, slots, resc.p, r_ops.p, pm);
    }
  }
  // the pair choice (without a hit anywhere: no rescued candidates)
  DevBuf<uint64_t> nmaps(n), moff(n + 1);
  launch_pair_select<Rec>(r, koff.p, cands.p, resc.p, rstatus.p, P, pp, pm, nmaps.p, nullptr, nullptr, nullptr, nullptr, nullptr, s);
  launch_scan(r, nmaps.p, n, moff.p, S.scratch.p, s);
  uint64_t nrec = 0;
  HIP_CHECK(hipMemcpyAsync(&nrec, moff.p + n, 8, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipMemcpyAsync(out.n_maps.data() + at_q, nmaps.p, n * 8, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
  require(nrec >= 1 && nrec <= n, "internal: the pair choice reports no record of a chunk with candidates, or more than one per read");
  DevBuf<Rec> maps(nrec);
  DevBuf<uint32_t> sel(nrec), ins(P);
  DevBuf<uint64_t> pos(want_pos ? 2 * nrec : 0);
  launch_pair_select<Rec>(r, koff.p, cands.p, resc.p, rstatus.p, P, pp, pm, nullptr, moff.p, maps.p, sel.p, want_pos ? pos.p : nullptr, ins.p, s);
  out.maps.resize(at_m + nrec);
  HIP_CHECK(hipMemcpyAsync(out.maps.data() + at_m, maps.p, nrec * sizeof(Rec), hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipMemcpyAsync(out.insert.data() + at_p, ins.p, P * 4, hipMemcpyDeviceToHost, s));
  if (want_pos) {
    out.pos.resize(at_m + nrec);
    HIP_CHECK(hipMemcpyAsync(out.pos.data() + at_m, pos.p, nrec * sizeof(awry_pos_t), hipMemcpyDeviceToHost, s));
  }
  std::vector<uint32_t> h_sel(want_cigar ? nrec : 0), h_cand_aln(want_cigar ? ncand : 0);
  if (want_cigar) {
    HIP_CHECK(hipMemcpyAsync(h_sel.data(), sel.p, nrec * 4, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(h_cand_aln.data(), cand_aln.p, ncand * 4, hipMemcpyDeviceToHost, s));
  }
  HIP_CHECK(hipStreamSynchronize(s));
  if (!want_cigar) return;
  // the CIGARs, in record order: the chain-derived records' alignments as a list of their own through the fill pass, the rescued
  // records' runs out of the aligner's slots
  std::vector<uint32_t> h_win;
  bool any_rescued = false;
  for (uint32_t at : h_sel) {
    if (at & PAIR_SEL_RESCUED) { any_rescued = true; continue; }
    require(at < ncand, "internal: a record names no candidate");
    h_win.push_back(h_cand_aln[at]);
  }
  const uint64_t nwin = h_win.size();
  std::vector<uint64_t> c_nops(nwin);
  std::vector<uint32_t> c_cigar, h_rops;
  std::vector<uint8_t> h_rnops;
  if (nwin) {
    DevBuf<uint32_t> d_win(nwin);
    HIP_CHECK(hipMemcpyAsync(d_win.p, h_win.data(), nwin * 4, hipMemcpyHostToDevice, s));
    fill_reported_cigars(r, text8, v, S, nops.p, d_win.p, nwin, band, md, (uint32_t)Lmax, c_nops.data(), c_cigar);
  }
  if (any_rescued) {
    require(resc.p != nullptr, "internal: a rescued record without a rescue pass");
    h_rops.resize(slots * ALIGN_MAX_OPS);
    h_rnops.resize(slots);
    HIP_CHECK(hipMemcpyAsync(h_rops.data(), r_ops.p, slots * ALIGN_MAX_OPS * 4, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(h_rnops.data(), r_nops.p, slots, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
  }
  uint64_t c = 0, c_at = 0;
  for (uint32_t at : h_sel) {
    if (at & PAIR_SEL_RESCUED) {
      const uint64_t w = at & ~PAIR_SEL_RESCUED;
      require(w < slots, "internal: a rescued record names no slot");
      out.n_ops.push_back(h_rnops[w]);
      out.cigar.insert(out.cigar.end(), h_rops.begin() + w * ALIGN_MAX_OPS, h_rops.begin() + w * ALIGN_MAX_OPS + h_rnops[w]);
    } else {
      out.n_ops.push_back(c_nops[c]);
      out.cigar.insert(out.cigar.end(), c_cigar.begin() + c_at, c_cigar.begin() + c_at + c_nops[c]);
      c_at += c_nops[c++];
    }
  }
  require(c_at == c_cigar.size(), "internal: the fill pass's runs do not cover the chain-derived records");
}

// awry_map_pairs_batch: shards, chunks and halves between pairs; results stitched in read order into pinned-pool arrays.  The
// out-pointers are written only when everything has succeeded.  awry_map_pairs_clip_batch is the same with the clipped modes and
// MapT = awry_map_clip_t.
template <class MapT>
void map_pairs_batch(awry_index* idx, const uint8_t* qbytes, const uint64_t* qoff, uint64_t n, uint32_t min_len, uint64_t max_hits, const ChainParams& P,
                     uint32_t chains_per_strand, uint32_t band, const AlignMode& md, const MapMode& mm, const PairMode& pm, const PairParams& pp,
                     uint64_t** map_off_out, MapT** maps_out, awry_pos_t** pos_out, uint64_t** cigar_off_out, uint32_t** cigar_out, uint8_t** status_out,
                     uint32_t** insert_out) {
  using PairHits = PairHitsOf<MapT>;
  if (idx->host.alphabet != NUCLEOTIDE) throw ArgError("mapping read pairs needs a nucleotide index");
  if (n % 2) throw ArgError("read pairs are interleaved: an odd number of reads");
  require_chain_index(idx->host.bwt_len);
  require_chain_align_lengths(qoff, n);
  const bool want_cigar = cigar_out != nullptr, want_pos = pos_out != nullptr;
  const uint64_t npairs = n / 2;
  std::vector<uint64_t> pair_off(npairs + 1);  // the pairs as the units that are sharded, chunked and halved
  for (uint64_t p = 0; p <= npairs; p++) pair_off[p] = qoff[2 * p];
  std::vector<PairHits> res(std::max<size_t>(1, idx->reps.size()));
  for_each_replica(idx, npairs, [&](Replica& r, Shard sh, int g) {
    HIP_CHECK(hipSetDevice(r.device));
    const uint8_t* text8 = edit_text(r);
    const auto sink = [&, g, text8](Replica& rr, const ChainOnDevice& v) {
      pair_chunk(rr, text8, v, chains_per_strand, (int)band, md, mm, pm, pp, want_pos, want_cigar, res[g]);
    };
    for (Shard c : chunk_queries(pair_off.data(), sh.lo, sh.hi, 4))  // a pair is four queries of the doubled batch
      halve_until_fits(c, [&](Shard h) { return chain_chunk(r, qbytes, qoff, Shard{2 * h.lo, 2 * h.hi}, min_len, max_hits, P, true, sink, 2); });
  });
  MBuf<uint64_t> moff, coff;
  MBuf<MapT> maps;
  MBuf<awry_pos_t> pos;
  MBuf<uint32_t> cg, ins;
  MBuf<uint8_t> st;
  const uint64_t total = stitch_offsets(res, &PairHits::n_maps, n, moff);
  for (auto& x : res)
    require((!want_pos || x.pos.size() == x.maps.size()) && (!want_cigar || x.n_ops.size() == x.maps.size()), "internal: the passes do not cover the records");
  require(stitch_size(res, &PairHits::maps) == total && stitch_size(res, &PairHits::insert) == npairs, "internal: shard results do not cover the records");
  if (status_out) stitch_concat(res, &PairHits::status, st);
  if (maps_out) stitch_concat(res, &PairHits::maps, maps);
  if (want_pos) stitch_concat(res, &PairHits::pos, pos);
  if (want_cigar) stitch_run_offsets(res, &PairHits::n_ops, total, stitch_concat(res, &PairHits::cigar, cg), coff);
  if (insert_out) stitch_concat(res, &PairHits::insert, ins);
  *map_off_out = moff.release();
  if (maps_out) *maps_out = maps.release();
  if (want_pos) *pos_out = pos.release();
  if (want_cigar) { *cigar_off_out = coff.release(); *cigar_out = cg.release(); }
  if (status_out) *status_out = st.release();
  if (insert_out) *insert_out = ins.release();
}

}  // namespace
