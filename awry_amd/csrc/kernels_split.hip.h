// kernels_split.hip.h -- split reads: the selection of a read's clipped alignments by query interval.  Segments (a primary and up
// to three supplementaries that explain different letters of the read), their secondaries, and a MAPQ per segment.  Included by
// kernels.hip.h after kernels_map.hip.h (it uses AlnClip, Chain, MapMode, MapKey / map_key, localise).
//
// No counterpart in the reference.  The definition is the one include/awry_hip.h states ("split reads"); in short, candidates,
// threshold and rank are the clipped map level's; a candidate's query interval [q_begin, q_end) follows from its clips, its strand
// and the read's length; the ranked list is walked once: a candidate whose text span intersects a better-ranked kept one of its
// strand is dropped, one that overlaps a segment by at least max_overlap percent of the shorter of the two is a secondary of the
// first such segment (and, if that segment has none yet, its MAPQ competitor), any other becomes a new segment while fewer than
// max_segments exist.
#pragma once

namespace awry {

constexpr int SPLIT_MAX_SEGMENTS = 4;         // AWRY_SPLIT_MAX_SEGMENTS
constexpr uint16_t MAP_SUPPLEMENTARY = 16;    // AWRY_MAP_SUPPLEMENTARY
constexpr uint32_t SPLIT_MAX_READ = 0xFFFFu;  // a longer read counts as this long: the interval is two 16-bit fields

struct MapSplitRec {  // == awry_map_split_t (checked in split_host.h): MapClipRec's fields, then the query interval and the segment
  uint64_t t_begin, t_end;
  uint32_t edits, chain_score, chain_index;
  uint8_t strand, mapq;
  uint16_t flags;
  int32_t score;
  uint16_t clip_left, clip_right;
  uint16_t q_begin, q_end, parent, reserved;
};

struct SplitParams { uint32_t max_segments = 1, max_secondary = 0, max_overlap = 50; };  // P, R2, O

// q_begin | q_end << 16 of an alignment on `strand` of a read of L <= SPLIT_MAX_READ letters, in the read's own orientation; both
// clips saturate at L, so any record gives 0 <= q_begin <= q_end <= L
__device__ __forceinline__ uint32_t split_interval(const AlnClip& a, uint32_t strand, uint32_t L) {
  const uint32_t lo = strand ? a.clip_right : a.clip_left, hi = strand ? a.clip_left : a.clip_right;
  const uint32_t qb = lo < L ? lo : L, r = L - (hi < L ? hi : L);
  return qb | (r > qb ? r : qb) << 16;
}

// One read per lane, grid-stride; candidates, slots and rank as in map_select_kernel<.., true>, the records re-read.  Pass one
// classifies: every round takes the smallest key among the open slots, drops it if its interval is empty or a kept slot of its strand
// has an intersecting span, else tests it against the segments so far (their intervals: four 16-bit fields in each of two words),
// first accepted first.  What is kept goes, in rank order k = 0, 1, .., into three words: ord (the slot), par (the segment index: its
// own for a segment) -- sixteen 4-bit entries each -- and a bit of segm for a segment.  sub holds, per segment, the slot of its first
// secondary (havesub: which have one).  The walk ends when nothing is open, or when nothing that follows can change the output: all
// max_segments segments exist, max_secondary secondaries are kept and (FILL) every segment has its sub.
// FILL = false: n_maps[i] = segments + min(max_secondary, secondaries), read_status[i] (nullable) as map_select_kernel writes it.
// FILL = true: pass two emits in rank order, segment x at map_off[i] + x, the k-th reported secondary behind the segments; per
// record (both nullable) sel[] = the alignment's index and pos[] = record and offset of t_begin; never a slot at or beyond
// map_off[i + 1].  The length of read i is qoff[qstride i + 1] - qoff[qstride i]: qstride 1 over the reads' own offsets, 2 over the
// doubled batch's.
template <bool FILL>
__global__ __launch_bounds__(256) void map_split_select_kernel(DevIndex ix, const uint64_t* __restrict__ aln_off, const AlnClip* __restrict__ alns,
                                                               const Chain* __restrict__ chains, const uint8_t* __restrict__ chain_status,
                                                               const uint64_t* __restrict__ qoff, uint32_t qstride, uint64_t n, uint32_t A, SplitParams sp,
                                                               uint64_t* __restrict__ n_maps, uint8_t* __restrict__ read_status,
                                                               const uint64_t* __restrict__ map_off, MapSplitRec* __restrict__ maps, uint32_t* __restrict__ sel,
                                                               uint64_t* __restrict__ pos, MapMode md) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  const uint32_t P = sp.max_segments, R2 = sp.max_secondary;
  const int32_t O = (int32_t)sp.max_overlap;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const uint64_t lo0 = aln_off[2 * i], lo1 = aln_off[2 * i + 1], hi1 = aln_off[2 * i + 2];
    const uint32_t c0 = (uint32_t)(lo1 - lo0 < A ? lo1 - lo0 : A), c1 = (uint32_t)(hi1 - lo1 < A ? hi1 - lo1 : A);
    const bool capped = chain_status && (chain_status[2 * i] == Q_SEED_CAP || chain_status[2 * i + 1] == Q_SEED_CAP);
    const uint64_t q0 = qoff[(uint64_t)qstride * i], q1 = qoff[(uint64_t)qstride * i + 1];
    const uint32_t L = q1 > q0 ? (q1 - q0 < (uint64_t)SPLIT_MAX_READ ? (uint32_t)(q1 - q0) : SPLIT_MAX_READ) : 0u;
    auto at = [&](uint32_t c) { return (c >> 3 ? lo1 : lo0) + (c & 7u); };
    uint32_t open = 0;  // candidate slots not yet taken
    for (uint32_t j = 0; j < c0; j++) open |= alns[lo0 + j].status == ALN_OK && alns[lo0 + j].score >= md.min_score ? 1u << j : 0u;
    for (uint32_t j = 0; j < c1; j++) open |= alns[lo1 + j].status == ALN_OK && alns[lo1 + j].score >= md.min_score ? 1u << (8 + j) : 0u;
    uint32_t kept = 0, nkept = 0, nseg = 0, nsec = 0, segm = 0, sub = 0, havesub = 0;
    uint64_t ord = 0, par = 0, seg_b = 0, seg_e = 0;
    const uint32_t all_subs = (1u << P) - 1u;
    while (open && !(nseg == P && nsec >= R2 && (!FILL || havesub == all_subs))) {
      uint32_t best = 0;
      MapKey bk{};
      bool have = false;
      for (uint32_t m = open; m; m &= m - 1) {
        const uint32_t c = (uint32_t)__ffs((int)m) - 1u;
        const uint64_t a = at(c);
        const MapKey k = map_key<true>(alns[a], chains[a].score, c);
        if (!have || k.before(bk)) { bk = k; best = c; have = true; }
      }
      open &= ~(1u << best);
      const AlnClip w = alns[at(best)];
      const uint32_t iv = split_interval(w, best >> 3, L);
      const int32_t qb = (int32_t)(iv & 0xFFFFu), qe = (int32_t)(iv >> 16);
      if (qe == qb) continue;  // explains no letter: not kept, and no part in redundancy
      bool redundant = false;
      for (uint32_t m = kept & (best >> 3 ? 0xFF00u : 0x00FFu); m; m &= m - 1) {
        const AlnClip o = alns[at((uint32_t)__ffs((int)m) - 1u)];
        redundant |= (w.t_begin > o.t_begin ? w.t_begin : o.t_begin) < (w.t_end < o.t_end ? w.t_end : o.t_end);
      }
      if (redundant) continue;
      uint32_t x = SPLIT_MAX_SEGMENTS;  // the first accepted segment that c overlaps
#pragma unroll
      for (int y = SPLIT_MAX_SEGMENTS - 1; y >= 0; y--) {
        const int32_t gb = (int32_t)(seg_b >> (16 * y) & 0xFFFFu), ge = (int32_t)(seg_e >> (16 * y) & 0xFFFFu);
        const int32_t ov = (qe < ge ? qe : ge) - (qb > gb ? qb : gb), shorter = qe - qb < ge - gb ? qe - qb : ge - gb;
        if ((uint32_t)y < nseg && ov > 0 && 100 * ov >= O * shorter) x = (uint32_t)y;
      }
      if (x == (uint32_t)SPLIT_MAX_SEGMENTS) {
        if (nseg >= P) continue;  // the segment cap: dropped, not kept
        seg_b |= (uint64_t)(uint32_t)qb << (16 * nseg);
        seg_e |= (uint64_t)(uint32_t)qe << (16 * nseg);
        segm |= 1u << nkept;
        x = nseg++;
      } else {
        if (!(havesub >> x & 1u)) { havesub |= 1u << x; sub |= best << (4 * x); }  // ranked: the best competitor for those letters
        nsec++;
      }
      ord |= (uint64_t)best << (4 * nkept);
      par |= (uint64_t)x << (4 * nkept);
      kept |= 1u << best;
      nkept++;
    }
    const uint32_t rsec = nsec < R2 ? nsec : R2;
    if (!FILL) {
      n_maps[i] = nseg + rsec;
      if (read_status) read_status[i] = capped ? Q_SEED_CAP : Q_OK;
      continue;
    }
    const uint64_t out = map_off[i], cap = map_off[i + 1] - out;
    uint32_t si = 0, ci = 0;
    for (uint32_t k = 0; k < nkept; k++) {
      const uint32_t c = (uint32_t)(ord >> (4 * k)) & 15u, x = (uint32_t)(par >> (4 * k)) & 15u;
      const bool is_seg = segm >> k & 1u;
      if (!is_seg && ci >= rsec) continue;  // only the report is cut
      const uint32_t slot = is_seg ? si++ : nseg + ci++;
      if (slot >= cap) continue;
      const uint64_t a = at(c);
      const AlnClip w = alns[a];
      const uint32_t iv = split_interval(w, c >> 3, L);
      uint32_t mapq = 0;
      if (is_seg && !capped) {
        mapq = MAP_MAPQ_MAX;
        if (havesub >> x & 1u) {
          const int64_t d = 10 * ((int64_t)w.score - (int64_t)alns[at(sub >> (4 * x) & 15u)].score) / (int64_t)md.mapq_div;  // (>= 0: the rank order)
          mapq = d < (int64_t)MAP_MAPQ_MAX ? (uint32_t)d : MAP_MAPQ_MAX;
        }
      }
      const uint16_t fl = (uint16_t)(is_seg ? (x ? MAP_SUPPLEMENTARY : 0) : MAP_SECONDARY);
      maps[out + slot] = MapSplitRec{w.t_begin, w.t_end, w.edits, chains[a].score, c & 7u, (uint8_t)(c >> 3), (uint8_t)mapq, fl, w.score, w.clip_left, w.clip_right,
                                     (uint16_t)(iv & 0xFFFFu), (uint16_t)(iv >> 16), (uint16_t)x, (uint16_t)0};
      if (sel) sel[out + slot] = (uint32_t)a;
      if (pos) localise(ix, w.t_begin < ix.bwt_len ? w.t_begin : ix.bwt_len - 1, pos + 2 * (out + slot));  // (a caller's record past the text: the last record)
    }
  }
}

}  // namespace awry
