// split_host.h -- the driver of awry_map_split_batch: map_host.h's chunk and batch drivers (select_chunk, map_batch_over) with the
// split selection (kernels_split.hip.h) in the place of map_select.  split_chunk is a sink of chain_chunk over the doubled batch,
// like map_chunk: the candidates stage in the clipped mode (align_candidates), the split selection per read (count pass, scan, fill
// pass), and the CIGAR fill over the reported alignments (fill_reported_cigars).  The reads, the seeding parameters and the result
// arrays arrive in the family's bundles (Reads, Seeding, MapOut).
// A part of awry_hip.hip (one translation unit): included there, in order, after map_host.h, and not on its own.
#pragma once

namespace {

// ---- split reads (kernels_split.hip.h) ------------------------------------------------------------------------------------------------

static_assert(sizeof(MapSplitRec) == sizeof(awry_map_split_t) && sizeof(awry_map_split_t) == 48, "the kernel writes awry_map_split_t records");
static_assert(offsetof(awry_map_split_t, t_begin) == offsetof(awry_map_clip_t, t_begin) && offsetof(awry_map_split_t, t_end) == offsetof(awry_map_clip_t, t_end) &&
                  offsetof(awry_map_split_t, edits) == offsetof(awry_map_clip_t, edits) && offsetof(awry_map_split_t, chain_score) == offsetof(awry_map_clip_t, chain_score) &&
                  offsetof(awry_map_split_t, chain_index) == offsetof(awry_map_clip_t, chain_index) && offsetof(awry_map_split_t, strand) == offsetof(awry_map_clip_t, strand) &&
                  offsetof(awry_map_split_t, mapq) == offsetof(awry_map_clip_t, mapq) && offsetof(awry_map_split_t, flags) == offsetof(awry_map_clip_t, flags) &&
                  offsetof(awry_map_split_t, score) == offsetof(awry_map_clip_t, score) && offsetof(awry_map_split_t, clip_left) == offsetof(awry_map_clip_t, clip_left) &&
                  offsetof(awry_map_split_t, clip_right) == offsetof(awry_map_clip_t, clip_right),
              "awry_map_split_t begins with awry_map_clip_t's eleven fields at their offsets");
static_assert(offsetof(awry_map_split_t, q_begin) == 40 && offsetof(awry_map_split_t, q_end) == 42 && offsetof(awry_map_split_t, parent) == 44 &&
                  offsetof(awry_map_split_t, reserved) == 46 && offsetof(MapSplitRec, q_begin) == 40 && offsetof(MapSplitRec, q_end) == 42 &&
                  offsetof(MapSplitRec, parent) == 44 && offsetof(MapSplitRec, reserved) == 46 && offsetof(MapSplitRec, flags) == offsetof(awry_map_split_t, flags) &&
                  offsetof(MapSplitRec, score) == offsetof(awry_map_split_t, score) && offsetof(MapSplitRec, mapq) == offsetof(awry_map_split_t, mapq),
              "the query interval and the parent follow the clips");
static_assert(SPLIT_MAX_SEGMENTS == AWRY_SPLIT_MAX_SEGMENTS && MAP_SUPPLEMENTARY == AWRY_MAP_SUPPLEMENTARY && 4 * 2 * MAP_MAX_CHAINS <= 64,
              "the kernel's limits are the header's, and sixteen 4-bit entries fit a word");

SplitParams split_params(uint64_t chains_per_strand, uint64_t max_segments, uint64_t max_secondary, uint32_t max_overlap, uint32_t band) {
  if (chains_per_strand < 1 || chains_per_strand > (uint64_t)MAP_MAX_CHAINS) throw ArgError("chains_per_strand must be in 1..8 (AWRY_MAP_MAX_CHAINS)");
  if (max_segments < 1 || max_segments > (uint64_t)SPLIT_MAX_SEGMENTS) throw ArgError("max_segments must be in 1..4 (AWRY_SPLIT_MAX_SEGMENTS)");
  if (max_secondary > 2 * chains_per_strand) throw ArgError("max_secondary must be in 0 .. 2 * chains_per_strand");
  if (max_overlap < 1 || max_overlap > 100) throw ArgError("max_overlap is a percentage in 1..100");
  require_chain_align_args(1, band);
  return SplitParams{(uint32_t)max_segments, (uint32_t)max_secondary, max_overlap};
}

// select_chunk (map_host.h) with the split selection; the read lengths are those of the chunk's doubled batch, L_i = off[2i+1] - off[2i]
void split_chunk(Replica& r, const ChainOnDevice& v, const ChunkAlign& ca, const SplitParams& sp, const MapMode& mm, MapHitsOf<awry_map_split_t>& out) {
  const uint64_t n = v.c.hi - v.c.lo;
  select_chunk(r, v, ca, out,
               [&](const SelectedChains& S, const void* alns, uint64_t* n_maps, uint8_t* read_status, const uint64_t* map_off, void* maps, uint32_t* sel, uint64_t* pos) {
                 launch_map_split_select(r, S.aoff.p, static_cast<const AlnClip*>(alns), S.chains.p, v.status, v.cb.off.p, 2, n, ca.A, sp, mm, n_maps, read_status,
                                         map_off, static_cast<MapSplitRec*>(maps), sel, pos, r.stream);
               });
}

// awry_map_split_batch: map_batch's shards, halves and stitching (map_batch_over) around split_chunk
void split_batch(awry_index* idx, const Reads& q, const Seeding& sc, uint32_t chains_per_strand, const SplitParams& sp, uint32_t band, const AlignMode& md,
                 const MapMode& mm, const MapOut<awry_map_split_t>& out) {
  map_batch_over(idx, q, sc, chains_per_strand, band, md, out,
                 [&](Replica& r, const ChainOnDevice& v, const ChunkAlign& ca, MapHitsOf<awry_map_split_t>& hits) { split_chunk(r, v, ca, sp, mm, hits); });
}

}  // namespace
