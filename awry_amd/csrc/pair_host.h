// pair_host.h -- the driver of awry_map_pairs_batch, a sink of chain_chunk over the doubled batch of 2 P reads (chain_host.h, both
// strands) and a client of map_host.h's stages: align_candidates, MapHitsOf with `insert`, fill_reported_cigars, stitch_map_hits.
// The pairs' own, top to bottom: kept_lists -- every read's candidates as records (map_select at max_report = 2 A); mate_rescue --
// the rescue windows, the edit scan over them and the aligner over each window's best hit (edit_host.h's launchers), the rescued
// candidates; merge_pair_cigars -- chain-derived records through the fill pass, rescued ones out of the aligner's fixed-stride
// runs; pair_chunk -- those three around the pair choice (count pass, scan, fill pass); map_pairs_batch -- shards between pairs.
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

template <class Rec>
struct KeptLists {  // every read's candidates in rank order, as records on the device
  DevBuf<uint64_t> nkept, koff;  // per read
  DevBuf<uint8_t> rstatus;       // per read: Q_OK or Q_SEED_CAP
  DevBuf<Rec> cands;             // the ncand candidates
  DevBuf<uint32_t> cand_aln;     // per candidate: the index of its alignment among C's
  uint64_t ncand = 0;
};

// map_chunk's selection at max_report = 2 A, so that every kept candidate of a read is a record on the device (count pass, scan, fill
// pass; the copy of the reads' status into h_status[n] rides on its one wait).  Without a candidate `cands` and `cand_aln` stay empty.
template <bool CLIP>
KeptLists<MapRecOf<CLIP>> kept_lists(Replica& r, const ChainOnDevice& v, const ChunkAlign& ca, const Candidates<CLIP>& C, const MapMode& mm, uint8_t* h_status) {
  const hipStream_t s = r.stream;
  const uint64_t n = v.c.hi - v.c.lo;
  const SelectedChains& S = C.S;
  KeptLists<MapRecOf<CLIP>> K;
  K.nkept.alloc(n); K.koff.alloc(n + 1); K.rstatus.alloc(n);
  launch_map_select(r, S.aoff.p, C.alns.p, S.chains.p, v.status, n, ca.A, 2 * ca.A, mm, K.nkept.p, K.rstatus.p, nullptr, nullptr, nullptr, nullptr, s);
  scan_with_total(r, K.nkept.p, n, K.koff.p, S.scratch.p, &K.ncand, s);
  HIP_CHECK(hipMemcpyAsync(h_status, K.rstatus.p, n, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
  require(K.ncand <= S.total, "internal: more candidates kept than aligned");
  if (!K.ncand) return K;
  K.cands.alloc(K.ncand); K.cand_aln.alloc(K.ncand);
  launch_map_select(r, S.aoff.p, C.alns.p, S.chains.p, v.status, n, ca.A, 2 * ca.A, mm, nullptr, nullptr, K.koff.p, K.cands.p, K.cand_aln.p, nullptr, s);
  return K;
}

template <class Rec>
struct MateRescue {  // what the rescue leaves on the device until the chunk is done; without a hit anywhere `resc` is empty
  uint64_t slots = 0;  // windows: rescue_anchors per read
  DevBuf<Rec> resc;    // per slot: the rescued candidate
  DevBuf<uint32_t> win_query, win_count, sub_query, sub_count, text_len, r_ops;  // (r_ops: the aligner's runs, ALIGN_MAX_OPS per slot)
  DevBuf<uint64_t> win_first, n_sub, sub_off, sscratch, sub_first, n_hits, hit_off, hscratch, hit_gpos, best_gpos;
  DevBuf<uint8_t> hit_edits, best_edits, r_nops;
};

// The rescue windows of the kept lists' anchors, cut for the scan; the edit scan over them (count pass, scan, fill pass: edit_host.h's
// launchers); the best hit of each window; the aligner over it; the rescued candidates under pm.
template <class Rec>
MateRescue<Rec> mate_rescue(Replica& r, const ChainOnDevice& v, const ChunkAlign& ca, const KeptLists<Rec>& K, const PairParams& pp, const PairMode& pm) {
  const hipStream_t s = r.stream;
  const uint64_t n = v.c.hi - v.c.lo, n2 = 2 * n, P = n / 2;
  const int k = (int)pp.rescue_edits;
  uint64_t Lresc = 0;  // the longest read the edit scan takes
  for (uint64_t i = 0; i < n2; i += 2) {
    const uint64_t L = v.cb.h_off[i + 1] - v.cb.h_off[i];
    if (L <= (uint64_t)EDIT_MAX_LEN) Lresc = std::max(Lresc, L);
  }
  MateRescue<Rec> M;
  const uint64_t slots = M.slots = n * pp.rescue_anchors;
  if (!slots || Lresc <= (uint64_t)k) return M;
  // the masks per query of the doubled batch, at the words the longest rescuable read needs: a longer read has no window, and the
  // scan takes no query of more than 64 W letters
  const int W = (int)((Lresc + 63) / 64);
  M.win_query.alloc(slots); M.win_count.alloc(slots); M.win_first.alloc(slots);
  M.n_sub.alloc(slots); M.sub_off.alloc(slots + 1); M.sscratch.alloc(scan_tiles(slots) + 1);
  launch_pair_windows(r, K.koff.p, K.cands.p, v.cb.off.p, 2, P, pp, M.win_query.p, M.win_first.p, M.win_count.p, s);
  const uint32_t sub = pair_sub_window();
  flat_launch(r, s, slots, pair_sub_windows_kernel<false>, M.win_query.p, M.win_first.p, M.win_count.p, slots, sub, M.n_sub.p, nullptr, nullptr, nullptr, nullptr);
  uint64_t m = 0, nhits = 0;
  scan_with_total(r, M.n_sub.p, slots, M.sub_off.p, M.sscratch.p, &m, s);
  HIP_CHECK(hipStreamSynchronize(s));
  if (m) {
    M.sub_query.alloc(m); M.sub_count.alloc(m); M.sub_first.alloc(m); M.n_hits.alloc(m); M.hit_off.alloc(m + 1); M.hscratch.alloc(scan_tiles(m) + 1);
    flat_launch(r, s, slots, pair_sub_windows_kernel<true>, M.win_query.p, M.win_first.p, M.win_count.p, slots, sub, nullptr, M.sub_off.p, M.sub_query.p,
                M.sub_first.p, M.sub_count.p);
    launch_edit_windows(r, ca.text8, v.cb.q.p, v.cb.off.p, M.sub_query.p, M.sub_first.p, M.sub_count.p, m, k, W, n2, M.n_hits.p, nullptr, nullptr, nullptr, s);
    scan_with_total(r, M.n_hits.p, m, M.hit_off.p, M.hscratch.p, &nhits, s);
    HIP_CHECK(hipStreamSynchronize(s));
  }
  if (!nhits) return M;
  M.hit_gpos.alloc(nhits); M.hit_edits.alloc(nhits); M.best_gpos.alloc(slots); M.best_edits.alloc(slots);
  M.text_len.alloc(slots); M.r_nops.alloc(slots); M.r_ops.alloc(slots * ALIGN_MAX_OPS); M.resc.alloc(slots);
  launch_edit_windows(r, ca.text8, v.cb.q.p, v.cb.off.p, M.sub_query.p, M.sub_first.p, M.sub_count.p, m, k, W, n2, nullptr, M.hit_off.p, M.hit_gpos.p,
                      M.hit_edits.p, s);
  flat_launch(r, s, slots, pair_best_hit_kernel, M.sub_off.p, M.hit_off.p, M.hit_gpos.p, M.hit_edits.p, slots, M.best_gpos.p, M.best_edits.p);
  launch_edit_align(r, ca.text8, v.cb.q.p, v.cb.off.p, M.win_query.p, M.best_gpos.p, M.best_edits.p, slots, k, (uint32_t)Lresc, M.text_len.p, M.r_nops.p,
                    M.r_ops.p, s);
  flat_launch(r, s, slots, pair_rescued_kernel<Rec>, M.win_query.p, M.best_gpos.p, M.best_edits.p, M.text_len.p, M.r_nops.p, slots, M.resc.p, M.r_ops.p, pm);
  return M;
}

// The CIGARs in record order (h_sel[k]: record k's candidate, or PAIR_SEL_RESCUED | its slot): the chain-derived records' through the
// fill pass (fill_reported_cigars, map_host.h), the rescued records' out of the aligner's fixed-stride slots, merged on the host.
template <bool CLIP>
void merge_pair_cigars(Replica& r, const ChainOnDevice& v, const ChunkAlign& ca, const Candidates<CLIP>& C, const MateRescue<MapRecOf<CLIP>>& M,
                       const std::vector<uint32_t>& h_sel, const std::vector<uint32_t>& h_cand_aln, std::vector<uint64_t>& n_ops, std::vector<uint32_t>& cigar) {
  const hipStream_t s = r.stream;
  const uint64_t slots = M.slots;
  std::vector<uint32_t> h_win;
  bool any_rescued = false;
  for (uint32_t at : h_sel) {
    if (at & PAIR_SEL_RESCUED) { any_rescued = true; continue; }
    require(at < h_cand_aln.size(), "internal: a record names no candidate");
    h_win.push_back(h_cand_aln[at]);
  }
  const uint64_t nwin = h_win.size();
  std::vector<uint64_t> c_nops(nwin);
  std::vector<uint32_t> c_cigar, h_rops;
  std::vector<uint8_t> h_rnops;
  if (nwin) {
    DevBuf<uint32_t> d_win(nwin);
    HIP_CHECK(hipMemcpyAsync(d_win.p, h_win.data(), nwin * 4, hipMemcpyHostToDevice, s));
    fill_reported_cigars(r, v, ca, C, d_win.p, nwin, c_nops.data(), c_cigar);
  }
  if (any_rescued) {
    require(M.resc.p != nullptr, "internal: a rescued record without a rescue pass");
    h_rops.resize(slots * ALIGN_MAX_OPS);
    h_rnops.resize(slots);
    HIP_CHECK(hipMemcpyAsync(h_rops.data(), M.r_ops.p, slots * ALIGN_MAX_OPS * 4, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(h_rnops.data(), M.r_nops.p, slots, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
  }
  uint64_t c = 0, c_at = 0;
  for (uint32_t at : h_sel) {
    if (at & PAIR_SEL_RESCUED) {
      const uint64_t w = at & ~PAIR_SEL_RESCUED;
      require(w < slots, "internal: a rescued record names no slot");
      n_ops.push_back(h_rnops[w]);
      cigar.insert(cigar.end(), h_rops.begin() + w * ALIGN_MAX_OPS, h_rops.begin() + w * ALIGN_MAX_OPS + h_rnops[w]);
    } else {
      n_ops.push_back(c_nops[c]);
      cigar.insert(cigar.end(), c_cigar.begin() + c_at, c_cigar.begin() + c_at + c_nops[c]);
      c_at += c_nops[c++];
    }
  }
  require(c_at == c_cigar.size(), "internal: the fill pass's runs do not cover the chain-derived records");
}

// One chunk of whole pairs, from where chain_chunk's fill pass leaves the doubled batch (4 queries a pair): the candidates, the kept
// lists, the mate rescue, the pair choice (count pass, scan, fill pass) with the copy-out, and the chosen records' CIGARs, appended to
// `out`.  MapT is the record of the mode: ca.md for the alignment, mm for the kept lists, pm for the rescue and the pair choice.
template <class MapT>
void pair_chunk(Replica& r, const ChainOnDevice& v, const ChunkAlign& ca, const MapMode& mm, const PairMode& pm, const PairParams& pp, MapHitsOf<MapT>& out) {
  constexpr bool CLIP = std::is_same_v<MapT, awry_map_clip_t>;
  using Rec = MapRecOf<CLIP>;
  require(ca.md.clip == CLIP && mm.clip == CLIP && pm.clip == CLIP, "internal: the pair records are not the mode's");
  const hipStream_t s = r.stream;
  const uint64_t n = v.c.hi - v.c.lo, P = n / 2;
  require(n % 2 == 0, "internal: a chunk of read pairs holds an odd number of reads");
  const Candidates<CLIP> C = align_candidates<CLIP>(r, v, ca);
  const size_t at_q = out.n_maps.size(), at_m = out.maps.size(), at_p = out.insert.size();
  out.n_maps.resize(at_q + n); out.status.resize(at_q + n); out.insert.resize(at_p + P);  // (zeros: what a chunk without a candidate reports)
  const KeptLists<Rec> K = kept_lists(r, v, ca, C, mm, out.status.data() + at_q);
  if (!K.ncand) return;
  const MateRescue<Rec> M = mate_rescue(r, v, ca, K, pp, pm);
  // the pair choice (without a hit anywhere: no rescued candidates)
  DevBuf<uint64_t> nmaps(n), moff(n + 1);
  launch_pair_select<Rec>(r, K.koff.p, K.cands.p, M.resc.p, K.rstatus.p, P, pp, pm, nmaps.p, nullptr, nullptr, nullptr, nullptr, nullptr, s);
  uint64_t nrec = 0;
  scan_with_total(r, nmaps.p, n, moff.p, C.S.scratch.p, &nrec, s);
  HIP_CHECK(hipMemcpyAsync(out.n_maps.data() + at_q, nmaps.p, n * 8, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
  require(nrec >= 1 && nrec <= n, "internal: the pair choice reports no record of a chunk with candidates, or more than one per read");
  DevBuf<Rec> maps(nrec);
  DevBuf<uint32_t> sel(nrec), ins(P);
  DevBuf<uint64_t> pos(ca.want_pos ? 2 * nrec : 0);
  launch_pair_select<Rec>(r, K.koff.p, K.cands.p, M.resc.p, K.rstatus.p, P, pp, pm, nullptr, moff.p, maps.p, sel.p, ca.want_pos ? pos.p : nullptr, ins.p, s);
  out.maps.resize(at_m + nrec);
  HIP_CHECK(hipMemcpyAsync(out.maps.data() + at_m, maps.p, nrec * sizeof(Rec), hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipMemcpyAsync(out.insert.data() + at_p, ins.p, P * 4, hipMemcpyDeviceToHost, s));
  if (ca.want_pos) {
    out.pos.resize(at_m + nrec);
    HIP_CHECK(hipMemcpyAsync(out.pos.data() + at_m, pos.p, nrec * sizeof(awry_pos_t), hipMemcpyDeviceToHost, s));
  }
  std::vector<uint32_t> h_sel(ca.want_cigar ? nrec : 0), h_cand_aln(ca.want_cigar ? K.ncand : 0);
  if (ca.want_cigar) {
    HIP_CHECK(hipMemcpyAsync(h_sel.data(), sel.p, nrec * 4, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(h_cand_aln.data(), K.cand_aln.p, K.ncand * 4, hipMemcpyDeviceToHost, s));
  }
  HIP_CHECK(hipStreamSynchronize(s));
  if (ca.want_cigar) merge_pair_cigars(r, v, ca, C, M, h_sel, h_cand_aln, out.n_ops, out.cigar);
}

// awry_map_pairs_batch (MapT = awry_map_clip_t: awry_map_pairs_clip_batch): shards, chunks and halves between pairs, the units here
template <class MapT>
void map_pairs_batch(awry_index* idx, const Reads& q, const Seeding& sc, uint32_t chains_per_strand, uint32_t band, const AlignMode& md, const MapMode& mm,
                     const PairMode& pm, const PairParams& pp, const MapOut<MapT>& out) {
  if (idx->host.alphabet != NUCLEOTIDE) throw ArgError("mapping read pairs needs a nucleotide index");
  if (q.n % 2) throw ArgError("read pairs are interleaved: an odd number of reads");
  require_chain_index(idx->host.bwt_len);
  require_chain_align_lengths(q.off, q.n);
  const uint64_t npairs = q.n / 2;
  std::vector<uint64_t> pair_off(npairs + 1);  // the pairs as the units that are sharded, chunked and halved
  for (uint64_t p = 0; p <= npairs; p++) pair_off[p] = q.off[2 * p];
  std::vector<MapHitsOf<MapT>> res(std::max<size_t>(1, idx->reps.size()));
  for_each_replica(idx, npairs, [&](Replica& r, Shard sh, int g) {
    HIP_CHECK(hipSetDevice(r.device));
    const ChunkAlign ca{edit_text(r), chains_per_strand, (int)band, md, out.pos != nullptr, out.cigar != nullptr};
    const auto sink = [&, g](Replica& rr, const ChainOnDevice& v) { pair_chunk(rr, v, ca, mm, pm, pp, res[g]); };
    for (Shard c : chunk_queries(pair_off.data(), sh.lo, sh.hi, 4))  // a pair is four queries of the doubled batch
      halve_until_fits(c, [&](Shard h) { return chain_chunk(r, q, Shard{2 * h.lo, 2 * h.hi}, sc, true, sink, 2); });
  });
  stitch_map_hits(res, q.n, npairs, out);
}

}  // namespace
