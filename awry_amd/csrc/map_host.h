// map_host.h -- the driver of awry_map_batch, a sink of chain_chunk over the doubled batch (chain_host.h, both strands), and the
// stages split_host.h and pair_host.h share with it.  Top to bottom: align_candidates -- with chains and members still on the device,
// the first chains of every query (select_chains, chain_align_host.h) and the alignment count pass over all of them;
// fill_reported_cigars -- the gather of the reported alignments and the CIGAR fill over those only (fill_cigar), in sub-batches;
// select_chunk -- the candidates, the caller's selection per read (count pass, scan, fill pass), the copy-out, the CIGARs;
// stitch_map_hits -- the shards' results into the call's arrays; map_batch_over -- shards, chunks and halves around a chunk driver.
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

template <class MapT>  // awry_map_t, awry_map_clip_t in the clipped mode, awry_map_split_t for split reads
struct MapHitsOf {  // one shard's result, in read order
  std::vector<uint64_t> n_maps;  // per read
  std::vector<uint8_t> status;   // per read: Q_OK or Q_SEED_CAP
  std::vector<MapT> maps;
  std::vector<awry_pos_t> pos;
  std::vector<uint64_t> n_ops;   // per record
  std::vector<uint32_t> cigar;   // the runs, back to back
  std::vector<uint32_t> insert;  // per pair (pair_host.h); empty for single-end calls
};

template <class MapT>  // the result arrays of a call: `off` always, the others where the caller wants them; `insert` (per pair) in the pair calls only
struct MapOut { uint64_t** off; MapT** maps; awry_pos_t** pos; uint64_t** cigar_off; uint32_t** cigar; uint8_t** status; uint32_t** insert = nullptr; };

// what a chunk driver of the family aligns with (the replica's text, A = chains_per_strand, band, mode) and what it copies back
struct ChunkAlign { const uint8_t* text8; uint32_t A; int band; AlignMode md; bool want_pos, want_cigar; };

template <bool CLIP>
struct Candidates {  // the first chains of every query of the doubled batch, aligned: what select_chunk and pair_chunk (pair_host.h) start from
  SelectedChains S;
  DevBuf<uint64_t> nops;     // per chain of S: the CIGAR runs of its alignment
  DevBuf<AlnOf<CLIP>> alns;  // per chain of S: its alignment record
  uint32_t Lmax = 1;         // the longest query
};

// From where chain_chunk's fill pass leaves the doubled batch: the first min(n_chains, A) chains of each of the 2 n queries and
// the alignment count pass over all of them in sub-batches (before anything else: a selection needs every record).  Without a chain
// one element of each array is allocated: the selection's count pass still runs, and writes the zero counts and the reads' status.
template <bool CLIP>
Candidates<CLIP> align_candidates(Replica& r, const ChainOnDevice& v, const ChunkAlign& ca) {
  require(ca.md.clip == CLIP, "internal: the map records are not the mode's");
  const uint64_t n2 = 2 * (v.c.hi - v.c.lo);
  Candidates<CLIP> C;
  for (uint64_t i = 0; i < n2; i++) C.Lmax = (uint32_t)std::max<uint64_t>(C.Lmax, v.cb.h_off[i + 1] - v.cb.h_off[i]);
  SelectedChains& S = C.S;
  select_chains(r, v, n2, (uint64_t)ca.A, S);
  const uint64_t total = S.total;
  if (!total) { S.query.alloc(1); S.chains.alloc(1); S.moff.alloc(1); }
  C.nops.alloc(std::max<uint64_t>(total, 1));
  C.alns.alloc(std::max<uint64_t>(total, 1));
  if (total) {
    const uint64_t sub = std::min(chain_align_sub_batch(), total);
    for (uint64_t at = 0; at < total; at += sub)
      launch_chain_align(r, ca.text8, v.cb.q.p, v.cb.off.p, S.query.p + at, S.moff.p + at, S.members.p, std::min(sub, total - at), ca.band, ca.md, C.Lmax,
                         C.alns.p + at, C.nops.p + at, nullptr, nullptr, r.stream);
    S.release_scratch();
  }
  return C;
}

// The CIGAR fill over nwin reported alignments, d_win[k] = the index of record k's alignment among C's chains: the alignments as a
// chain list of their own (map_gather_kernel), then the fill pass over them only, in sub-batches.  n_ops[nwin] (host) receives the
// run counts, the runs are appended to `cigar`.
template <bool CLIP>
void fill_reported_cigars(Replica& r, const ChainOnDevice& v, const ChunkAlign& ca, const Candidates<CLIP>& C, const uint32_t* d_win, uint64_t nwin,
                          uint64_t* n_ops, std::vector<uint32_t>& cigar) {
  const hipStream_t s = r.stream;
  const SelectedChains& S = C.S;
  DevBuf<uint32_t> win_query(nwin);
  DevBuf<uint64_t> win_mcnt(nwin), win_nops(nwin), win_moff(nwin + 1), wscratch(scan_tiles(nwin) + 1);
  flat_launch(r, s, nwin, map_gather_kernel, d_win, nwin, S.query.p, S.moff.p, S.members.p, C.nops.p, win_query.p, win_mcnt.p, win_nops.p, nullptr, nullptr);
  uint64_t nwm = 0;
  scan_with_total(r, win_mcnt.p, nwin, win_moff.p, wscratch.p, &nwm, s);
  HIP_CHECK(hipMemcpyAsync(n_ops, win_nops.p, nwin * 8, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
  DevBuf<Seed> win_members(std::max<uint64_t>(nwm, 1));
  flat_launch(r, s, nwin, map_gather_kernel, d_win, nwin, S.query.p, S.moff.p, S.members.p, C.nops.p, nullptr, nullptr, nullptr, win_moff.p, win_members.p);
  const uint64_t sub = std::min(chain_align_sub_batch(), nwin);
  DevBuf<uint64_t> coff(sub + 1), cscratch(scan_tiles(sub) + 1);
  for (uint64_t at = 0; at < nwin; at += sub)
    fill_cigar(r, ca.text8, v.cb, win_query.p + at, win_moff.p + at, win_members.p, std::min(sub, nwin - at), ca.band, ca.md, C.Lmax, win_nops.p + at, coff.p,
               cscratch.p, cigar);
}

// One chunk: the candidates, the selection per read (count pass, scan, fill pass), and the CIGAR fill over the reported alignments,
// appended to `out`.  MapT is the record of ca.md's mode.  The selection is the caller's: select(S, alns, n_maps, read_status, map_off,
// maps, sel, pos) queues its count pass (map_off == nullptr) or its fill pass; map_chunk and split_chunk (split_host.h) pass theirs.
template <class MapT, class Select>
void select_chunk(Replica& r, const ChainOnDevice& v, const ChunkAlign& ca, MapHitsOf<MapT>& out, const Select& select) {
  constexpr bool CLIP = !std::is_same_v<MapT, awry_map_t>;
  const hipStream_t s = r.stream;
  const uint64_t n = v.c.hi - v.c.lo;
  const Candidates<CLIP> C = align_candidates<CLIP>(r, v, ca);
  const SelectedChains& S = C.S;
  // the selection: records per read, a scan, the records
  DevBuf<uint64_t> nmaps(n), moff(n + 1);
  DevBuf<uint8_t> rstatus(n);
  select(S, C.alns.p, nmaps.p, rstatus.p, nullptr, nullptr, nullptr, nullptr);
  uint64_t nwin = 0;
  scan_with_total(r, nmaps.p, n, moff.p, S.scratch.p, &nwin, s);
  const size_t at_q = out.n_maps.size(), at_m = out.maps.size();
  out.n_maps.resize(at_q + n); out.status.resize(at_q + n);
  HIP_CHECK(hipMemcpyAsync(out.n_maps.data() + at_q, nmaps.p, n * 8, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipMemcpyAsync(out.status.data() + at_q, rstatus.p, n, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
  require(nwin <= S.total, "internal: more records than candidates");
  if (!nwin) return;
  DevBuf<MapT> maps(nwin);  // (the kernels' records are the header's: the static_asserts)
  DevBuf<uint32_t> win(nwin);
  DevBuf<uint64_t> pos(ca.want_pos ? 2 * nwin : 0);
  select(S, C.alns.p, nullptr, nullptr, moff.p, maps.p, win.p, ca.want_pos ? pos.p : nullptr);
  out.maps.resize(at_m + nwin);
  HIP_CHECK(hipMemcpyAsync(out.maps.data() + at_m, maps.p, nwin * sizeof(MapT), hipMemcpyDeviceToHost, s));
  if (ca.want_pos) {
    out.pos.resize(at_m + nwin);
    HIP_CHECK(hipMemcpyAsync(out.pos.data() + at_m, pos.p, nwin * sizeof(awry_pos_t), hipMemcpyDeviceToHost, s));
  }
  if (!ca.want_cigar) {
    HIP_CHECK(hipStreamSynchronize(s));
    return;
  }
  out.n_ops.resize(at_m + nwin);
  fill_reported_cigars(r, v, ca, C, win.p, nwin, out.n_ops.data() + at_m, out.cigar);
}

// select_chunk with the selection of awry_map_batch (mm: end to end or clipped, as ca.md), R records per read at the most
template <class MapT>
void map_chunk(Replica& r, const ChainOnDevice& v, const ChunkAlign& ca, uint32_t R, const MapMode& mm, MapHitsOf<MapT>& out) {
  require(mm.clip == ca.md.clip, "internal: the map records are not the mode's");
  const uint64_t n = v.c.hi - v.c.lo;
  select_chunk(r, v, ca, out,
               [&](const SelectedChains& S, const void* alns, uint64_t* n_maps, uint8_t* read_status, const uint64_t* map_off, void* maps, uint32_t* sel, uint64_t* pos) {
                 launch_map_select(r, S.aoff.p, alns, S.chains.p, v.status, n, ca.A, R, mm, n_maps, read_status, map_off, maps, sel, pos, r.stream);
               });
}

// The shards' hits of n reads (n_pairs pairs; 0 for a single-end call) in read order, into pinned-pool arrays.  The out-pointers are
// written only when everything has succeeded: every array is stitched before the first is released.
template <class MapT>
void stitch_map_hits(const std::vector<MapHitsOf<MapT>>& res, uint64_t n, uint64_t n_pairs, const MapOut<MapT>& out) {
  using Hits = MapHitsOf<MapT>;
  const bool want_cigar = out.cigar != nullptr, want_pos = out.pos != nullptr;
  MBuf<uint64_t> moff, coff;
  MBuf<MapT> maps;
  MBuf<awry_pos_t> pos;
  MBuf<uint32_t> cg, ins;
  MBuf<uint8_t> st;
  const uint64_t total = stitch_offsets(res, &Hits::n_maps, n, moff);
  for (auto& x : res)
    require((!want_pos || x.pos.size() == x.maps.size()) && (!want_cigar || x.n_ops.size() == x.maps.size()), "internal: the passes do not cover the records");
  require(stitch_size(res, &Hits::maps) == total && stitch_size(res, &Hits::insert) == n_pairs, "internal: shard results do not cover the records");
  if (out.status) stitch_concat(res, &Hits::status, st);
  if (out.maps) stitch_concat(res, &Hits::maps, maps);
  if (want_pos) stitch_concat(res, &Hits::pos, pos);
  if (want_cigar) stitch_run_offsets(res, &Hits::n_ops, total, stitch_concat(res, &Hits::cigar, cg), coff);
  if (out.insert) stitch_concat(res, &Hits::insert, ins);
  *out.off = moff.release();
  if (out.maps) *out.maps = maps.release();
  if (want_pos) *out.pos = pos.release();
  if (want_cigar) { *out.cigar_off = coff.release(); *out.cigar = cg.release(); }
  if (out.status) *out.status = st.release();
  if (out.insert) *out.insert = ins.release();
}

// Shards over the replicas, chunks and halves between reads, results stitched in read order.  The chunk's work is the caller's:
// chunk(replica, chain view, ChunkAlign, the shard's hits) is map_chunk for map_batch below, split_chunk for split_batch (split_host.h).
template <class MapT, class Chunk>
void map_batch_over(awry_index* idx, const Reads& q, const Seeding& sc, uint32_t chains_per_strand, uint32_t band, const AlignMode& md, const MapOut<MapT>& out,
                    const Chunk& chunk) {
  if (idx->host.alphabet != NUCLEOTIDE) throw ArgError("mapping on both strands needs a nucleotide index");
  require_chain_index(idx->host.bwt_len);
  require_chain_align_lengths(q.off, q.n);
  std::vector<MapHitsOf<MapT>> res(std::max<size_t>(1, idx->reps.size()));
  for_each_replica(idx, q.n, [&](Replica& r, Shard sh, int g) {
    HIP_CHECK(hipSetDevice(r.device));
    const ChunkAlign ca{edit_text(r), chains_per_strand, (int)band, md, out.pos != nullptr, out.cigar != nullptr};
    const auto sink = [&, g](Replica& rr, const ChainOnDevice& v) { chunk(rr, v, ca, res[g]); };
    for (Shard c : chunk_queries(q.off, sh.lo, sh.hi, 2))  // halves between reads, never between a read's strands
      halve_until_fits(c, [&](Shard h) { return chain_chunk(r, q, h, sc, true, sink); });
  });
  stitch_map_hits(res, q.n, 0, out);
}

// awry_map_batch; awry_map_clip_batch is the same with the clipped modes and MapT = awry_map_clip_t
template <class MapT>
void map_batch(awry_index* idx, const Reads& q, const Seeding& sc, uint32_t chains_per_strand, uint32_t max_report, uint32_t band, const AlignMode& md,
               const MapMode& mm, const MapOut<MapT>& out) {
  map_batch_over(idx, q, sc, chains_per_strand, band, md, out,
                 [&](Replica& r, const ChainOnDevice& v, const ChunkAlign& ca, MapHitsOf<MapT>& hits) { map_chunk(r, v, ca, max_report, mm, hits); });
}

}  // namespace

