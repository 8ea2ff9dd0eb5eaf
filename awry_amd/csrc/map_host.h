// map_host.h -- the driver of awry_map_batch, a sink of chain_chunk over the doubled batch (chain_host.h, both strands): with
// chains and members still on the device, the first chains of every query (select_chains, chain_align_host.h), the alignment
// count pass over all of them, the selection per read (count pass, scan, fill pass), the gather of the reported alignments, the
// CIGAR fill over those only (fill_cigar), in sub-batches, and the copy-out
// A part of awry_hip.hip (one translation unit): included there, in order, after chain_align_host.h, and not on its own.
#pragma once

namespace {

// ---- map reads on both strands (kernels_map.hip.h) ----------------------------------------------------------------------------

static_assert(sizeof(MapRec) == sizeof(awry_map_t) && sizeof(awry_map_t) == 32 && offsetof(MapRec, t_end) == offsetof(awry_map_t, t_end) &&
                  offsetof(MapRec, edits) == offsetof(awry_map_t, edits) && offsetof(MapRec, chain_score) == offsetof(awry_map_t, chain_score) &&
                  offsetof(MapRec, chain_index) == offsetof(awry_map_t, chain_index) && offsetof(MapRec, strand) == offsetof(awry_map_t, strand) &&
                  offsetof(MapRec, mapq) == offsetof(awry_map_t, mapq) && offsetof(MapRec, flags) == offsetof(awry_map_t, flags),
              "the kernels write awry_map_t records");
static_assert(sizeof(MapClipRec) == sizeof(awry_map_clip_t) && sizeof(awry_map_clip_t) == 40 && offsetof(MapClipRec, flags) == offsetof(awry_map_clip_t, flags) &&
                  offsetof(MapClipRec, score) == offsetof(awry_map_clip_t, score) && offsetof(MapClipRec, clip_left) == offsetof(awry_map_clip_t, clip_left) &&
                  offsetof(MapClipRec, clip_right) == offsetof(awry_map_clip_t, clip_right) && offsetof(MapClipRec, mapq) == offsetof(awry_map_clip_t, mapq),
              "the kernels write awry_map_clip_t records");
static_assert(MAP_MAX_CHAINS == AWRY_MAP_MAX_CHAINS && MAP_SECONDARY == AWRY_MAP_SECONDARY && sizeof(awry_pos_t) == 16, "the kernels' limits are the header's");

void require_map_args(uint64_t chains_per_strand, uint64_t max_report, uint32_t band) {
  if (chains_per_strand < 1 || chains_per_strand > (uint64_t)MAP_MAX_CHAINS) throw ArgError("chains_per_strand must be in 1..8 (AWRY_MAP_MAX_CHAINS)");
  if (max_report < 1 || max_report > 2 * chains_per_strand) throw ArgError("max_report must be in 1 .. 2 * chains_per_strand");
  require_chain_align_args(1, band);
}

// the clipped selection's mode: the score threshold T >= 0 and the MAPQ divisor a + b
MapMode clip_map_mode(const AlignMode& md, uint32_t min_aln_score) {
  return MapMode{true, (int)std::min<uint32_t>(min_aln_score, 0x7FFFFFFFu), md.match + md.mismatch};
}

template <class MapT>  // awry_map_t, or awry_map_clip_t in the clipped mode
struct MapHitsOf {  // one shard's result, in read order
  std::vector<uint64_t> n_maps;  // per read
  std::vector<uint8_t> status;   // per read: Q_OK or Q_SEED_CAP
  std::vector<MapT> maps;
  std::vector<awry_pos_t> pos;
  std::vector<uint64_t> n_ops;  // per record
  std::vector<uint32_t> cigar;  // the runs, back to back
};
using MapHits = MapHitsOf<awry_map_t>;

// The CIGAR fill over nwin reported alignments, d_win[k] = the index of record k's alignment among S's chains (d_nops: their run
// counts): the alignments as a chain list of their own (map_gather_kernel), then the fill pass over them only, in sub-batches.
// n_ops[nwin] (host) receives the run counts, the runs are appended to `cigar`.  Shared with pair_chunk (pair_host.h).
void fill_reported_cigars(Replica& r, const uint8_t* text8, const ChainOnDevice& v, const SelectedChains& S, const uint64_t* d_nops, const uint32_t* d_win,
                          uint64_t nwin, int band, const AlignMode& md, uint32_t Lmax, uint64_t* n_ops, std::vector<uint32_t>& cigar) {
  const hipStream_t s = r.stream;
  DevBuf<uint32_t> win_query(nwin);
  DevBuf<uint64_t> win_mcnt(nwin), win_nops(nwin), win_moff(nwin + 1), wscratch(scan_tiles(nwin) + 1);
  flat_launch(r, s, nwin, map_gather_kernel, d_win, nwin, S.query.p, S.moff.p, S.members.p, d_nops, win_query.p, win_mcnt.p, win_nops.p, nullptr, nullptr);
  launch_scan(r, win_mcnt.p, nwin, win_moff.p, wscratch.p, s);
  uint64_t nwm = 0;
  HIP_CHECK(hipMemcpyAsync(&nwm, win_moff.p + nwin, 8, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipMemcpyAsync(n_ops, win_nops.p, nwin * 8, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
  DevBuf<Seed> win_members(std::max<uint64_t>(nwm, 1));
  flat_launch(r, s, nwin, map_gather_kernel, d_win, nwin, S.query.p, S.moff.p, S.members.p, d_nops, nullptr, nullptr, nullptr, win_moff.p, win_members.p);
  const uint64_t sub = std::min(chain_align_sub_batch(), nwin);
  DevBuf<uint64_t> coff(sub + 1), cscratch(scan_tiles(sub) + 1);
  for (uint64_t at = 0; at < nwin; at += sub)
    fill_cigar(r, text8, v.cb, win_query.p + at, win_moff.p + at, win_members.p, std::min(sub, nwin - at), band, md, Lmax, win_nops.p + at, coff.p, cscratch.p, cigar);
}

// One chunk, from where chain_chunk's fill pass leaves the doubled batch: the first min(n_chains, A) chains of each of the 2 n
// queries, the alignment count pass over all of them in sub-batches (before anything else: the selection needs every record),
// the selection per read, and the CIGAR fill over the reported alignments, appended to `out`.  MapT is the record of the mode (md
// for the alignment).  The selection is the caller's: select(S, alns, n_maps, read_status, map_off, maps, sel, pos) queues its count
// pass (map_off == nullptr) or its fill pass on the replica's stream; map_chunk below and split_chunk (split_host.h) each pass theirs.
template <class MapT, class Select>
void select_chunk(Replica& r, const uint8_t* text8, const ChainOnDevice& v, uint32_t A, int band, const AlignMode& md, bool want_pos, bool want_cigar,
                  MapHitsOf<MapT>& out, const Select& select) {
  constexpr bool CLIP = !std::is_same_v<MapT, awry_map_t>;
  require(md.clip == CLIP, "internal: the map records are not the mode's");
  const hipStream_t s = r.stream;
  const uint64_t n = v.c.hi - v.c.lo, n2 = 2 * n;
  uint64_t Lmax = 1;
  for (uint64_t i = 0; i < n2; i++) Lmax = std::max(Lmax, v.cb.h_off[i + 1] - v.cb.h_off[i]);
  SelectedChains S;
  select_chains(r, v, n2, (uint64_t)A, S);
  const uint64_t total = S.total;
  if (!total) { S.query.alloc(1); S.chains.alloc(1); S.moff.alloc(1); }  // launch_map_select still runs: it writes the zero counts and the reads' status
  DevBuf<uint64_t> nops(std::max<uint64_t>(total, 1));
  DevBuf<AlnOf<CLIP>> alns(std::max<uint64_t>(total, 1));
  if (total) {
    const uint64_t sub = std::min(chain_align_sub_batch(), total);
    for (uint64_t at = 0; at < total; at += sub)  // the count pass over every candidate: records and run counts stay on the device
      launch_chain_align(r, text8, v.cb.q.p, v.cb.off.p, S.query.p + at, S.moff.p + at, S.members.p, std::min(sub, total - at), band, md,
                         (uint32_t)Lmax, alns.p + at, nops.p + at, nullptr, nullptr, s);
    S.release_scratch();
  }
  // the selection: records per read, a scan, the records
  DevBuf<uint64_t> nmaps(n), moff(n + 1);
  DevBuf<uint8_t> rstatus(n);
  select(S, alns.p, nmaps.p, rstatus.p, nullptr, nullptr, nullptr, nullptr);
  launch_scan(r, nmaps.p, n, moff.p, S.scratch.p, s);
  uint64_t nwin = 0;
  const size_t at_q = out.n_maps.size(), at_m = out.maps.size();
  out.n_maps.resize(at_q + n);
  out.status.resize(at_q + n);
  HIP_CHECK(hipMemcpyAsync(&nwin, moff.p + n, 8, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipMemcpyAsync(out.n_maps.data() + at_q, nmaps.p, n * 8, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipMemcpyAsync(out.status.data() + at_q, rstatus.p, n, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
  require(nwin <= total, "internal: more records than candidates");
  if (!nwin) return;
  DevBuf<MapT> maps(nwin);  // (the kernels' records are the header's: the static_asserts)
  DevBuf<uint32_t> win(nwin);
  DevBuf<uint64_t> pos(want_pos ? 2 * nwin : 0);
  select(S, alns.p, nullptr, nullptr, moff.p, maps.p, win.p, want_pos ? pos.p : nullptr);
  out.maps.resize(at_m + nwin);
  HIP_CHECK(hipMemcpyAsync(out.maps.data() + at_m, maps.p, nwin * sizeof(MapT), hipMemcpyDeviceToHost, s));
  if (want_pos) {
    out.pos.resize(at_m + nwin);
    HIP_CHECK(hipMemcpyAsync(out.pos.data() + at_m, pos.p, nwin * sizeof(awry_pos_t), hipMemcpyDeviceToHost, s));
  }
  if (!want_cigar) {
    HIP_CHECK(hipStreamSynchronize(s));
    return;
  }
  out.n_ops.resize(at_m + nwin);
  fill_reported_cigars(r, text8, v, S, nops.p, win.p, nwin, band, md, (uint32_t)Lmax, out.n_ops.data() + at_m, out.cigar);
}

// select_chunk with the selection of awry_map_batch (mm: end to end or clipped, as md)
template <class MapT>
void map_chunk(Replica& r, const uint8_t* text8, const ChainOnDevice& v, uint32_t A, uint32_t R, int band, const AlignMode& md, const MapMode& mm, bool want_pos,
               bool want_cigar, MapHitsOf<MapT>& out) {
  require(mm.clip == md.clip, "internal: the map records are not the mode's");
  const uint64_t n = v.c.hi - v.c.lo;
  select_chunk(r, text8, v, A, band, md, want_pos, want_cigar, out,
               [&](const SelectedChains& S, const void* alns, uint64_t* n_maps, uint8_t* read_status, const uint64_t* map_off, void* maps, uint32_t* sel, uint64_t* pos) {
                 launch_map_select(r, S.aoff.p, alns, S.chains.p, v.status, n, A, R, mm, n_maps, read_status, map_off, maps, sel, pos, r.stream);
               });
}

// awry_map_batch: shards over the replicas, results stitched in read order into pinned-pool arrays.  The out-pointers are written
// only when everything has succeeded.  awry_map_clip_batch is the same with the clipped modes and MapT = awry_map_clip_t.
// The chunk's work is the caller's: chunk(replica, text8, chain view, want_pos, want_cigar, the shard's hits) is map_chunk for
// map_batch below and split_chunk for split_batch (split_host.h).
template <class MapT, class Chunk>
void map_batch_over(awry_index* idx, const uint8_t* qbytes, const uint64_t* qoff, uint64_t n, uint32_t min_len, uint64_t max_hits, const ChainParams& P,
                    uint64_t** map_off_out, MapT** maps_out, awry_pos_t** pos_out, uint64_t** cigar_off_out, uint32_t** cigar_out, uint8_t** status_out,
                    const Chunk& chunk) {
  if (idx->host.alphabet != NUCLEOTIDE) throw ArgError("mapping on both strands needs a nucleotide index");
  require_chain_index(idx->host.bwt_len);
  require_chain_align_lengths(qoff, n);
  const bool want_cigar = cigar_out != nullptr, want_pos = pos_out != nullptr;
  using Hits = MapHitsOf<MapT>;
  std::vector<Hits> res(std::max<size_t>(1, idx->reps.size()));
  for_each_replica(idx, n, [&](Replica& r, Shard sh, int g) {
    HIP_CHECK(hipSetDevice(r.device));
    const uint8_t* text8 = edit_text(r);
    const auto sink = [&, g, text8](Replica& rr, const ChainOnDevice& v) { chunk(rr, text8, v, want_pos, want_cigar, res[g]); };
    for (Shard c : chunk_queries(qoff, sh.lo, sh.hi, 2))  // halves between reads, never between a read's strands
      halve_until_fits(c, [&](Shard h) { return chain_chunk(r, qbytes, qoff, h, min_len, max_hits, P, true, sink); });
  });
  MBuf<uint64_t> moff, coff;
  MBuf<MapT> maps;
  MBuf<awry_pos_t> pos;
  MBuf<uint32_t> cg;
  MBuf<uint8_t> st;
  const uint64_t total = stitch_offsets(res, &Hits::n_maps, n, moff);
  for (auto& x : res)
    require((!want_pos || x.pos.size() == x.maps.size()) && (!want_cigar || x.n_ops.size() == x.maps.size()), "internal: the passes do not cover the records");
  require(stitch_size(res, &Hits::maps) == total, "internal: shard results do not cover the records");
  if (status_out) stitch_concat(res, &Hits::status, st);
  if (maps_out) stitch_concat(res, &Hits::maps, maps);
  if (want_pos) stitch_concat(res, &Hits::pos, pos);
  if (want_cigar) stitch_run_offsets(res, &Hits::n_ops, total, stitch_concat(res, &Hits::cigar, cg), coff);
  *map_off_out = moff.release();
  if (maps_out) *maps_out = maps.release();
  if (want_pos) *pos_out = pos.release();
  if (want_cigar) { *cigar_off_out = coff.release(); *cigar_out = cg.release(); }
  if (status_out) *status_out = st.release();
}

template <class MapT>
void map_batch(awry_index* idx, const uint8_t* qbytes, const uint64_t* qoff, uint64_t n, uint32_t min_len, uint64_t max_hits, const ChainParams& P,
               uint32_t chains_per_strand, uint32_t max_report, uint32_t band, const AlignMode& md, const MapMode& mm, uint64_t** map_off_out, MapT** maps_out,
               awry_pos_t** pos_out,
               uint64_t** cigar_off_out, uint32_t** cigar_out, uint8_t** status_out) {
  map_batch_over(idx, qbytes, qoff, n, min_len, max_hits, P, map_off_out, maps_out, pos_out, cigar_off_out, cigar_out, status_out,
                 [&](Replica& r, const uint8_t* text8, const ChainOnDevice& v, bool want_pos, bool want_cigar, MapHitsOf<MapT>& out) {
                   map_chunk(r, text8, v, chains_per_strand, max_report, (int)band, md, mm, want_pos, want_cigar, out);
                 });
}

}  // namespace
