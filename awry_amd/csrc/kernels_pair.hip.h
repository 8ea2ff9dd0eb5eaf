// kernels_pair.hip.h -- map read pairs: the window in which an unpaired placement expects its mate (mate rescue through the edit
// scan of edit_kernels.hip.h and the aligner of kernels_align.hip.h), the best hit of a window, the rescued candidate, and the
// choice of the pair of placements: insert-size pairing, pair MAPQ, the proper-pair flag.
// Included by kernels.hip.h after kernels_map.hip.h (it uses MapRec, localise, EDIT_MAX_LEN).
//
// No counterpart in the reference.  The definition is the one include/awry_hip.h states ("map read pairs"); in short, reads 2p and
// 2p + 1 are the mates of pair p, K_m is mate m's kept candidate list in rank order (map_select_kernel at max_report = 2 A), a
// placement of mate 0 and one of mate 1 are proper when they lie on opposite strands of one record, forward one first, with an
// outer distance in [min_insert, max_insert]; the first G candidates of a mate that are proper with nothing look for the other mate
// within k edits where the insert size allows it; the pair of smallest (edits + edits + U if improper) is reported.
// The clipped mode ("map read pairs, clipped") runs the same kernels over MapClipRec: the insert is measured between the mates' 5'
// ends projected through their clips, a rescued candidate carries the score of its runs, and the pair of largest (score + score - U
// if improper) is reported.
#pragma once

namespace awry {

constexpr uint32_t PAIR_MAX_INSERT = 1u << 20;   // AWRY_PAIR_MAX_INSERT
constexpr int PAIR_MAX_ANCHORS = 4;              // AWRY_PAIR_MAX_ANCHORS
constexpr uint32_t PAIR_CLIP_MAX_UNPAIRED = 16384; // AWRY_PAIR_CLIP_MAX_UNPAIRED: the largest score of a read, 1024 letters at a = 16
constexpr uint32_t PAIR_NO_CHAIN = 0xFFFFFFFFu;  // AWRY_PAIR_NO_CHAIN: chain_index of a rescued candidate
constexpr uint32_t PAIR_NO_RESCUE = 0xFFFFFFFFu; // edits of a d_resc slot that holds no candidate
constexpr uint32_t PAIR_SEL_RESCUED = 0x80000000u;
constexpr uint16_t MAP_PROPER_PAIR = 2, MAP_RESCUED = 4, MAP_MATE_UNMAPPED = 8;
constexpr uint8_t PAIR_NO_HIT = 0xFF;            // best_edits of a window without a hit: above every k, so the aligner skips it

struct PairParams {
  uint32_t min_insert, max_insert, unpaired_penalty, rescue_anchors, rescue_edits;
};

// The mode of the pair kernels: end to end (the default, over MapRec), or clipped (over MapClipRec) with the weights a, b, g that
// score a rescued candidate's runs, the score threshold T it must reach, and the MAPQ divisor a + b.
struct PairMode { bool clip = false; int match = 0, mismatch = 0, gap = 0, min_score = 0, mapq_div = 1; };
template <class Rec> constexpr bool pair_clipped = std::is_same_v<Rec, MapClipRec>;

// fb(x) and ve(x): the text position of the 5' end of a forward (reverse) placement -- in the clipped mode projected through the clip
// on that side, so possibly outside the record or below 0; used only in differences
template <class Rec> __device__ __forceinline__ long long pair_fb(const Rec& x) {
  if constexpr (pair_clipped<Rec>) return (long long)x.t_begin - (long long)x.clip_left;
  else return (long long)x.t_begin;
}
template <class Rec> __device__ __forceinline__ long long pair_ve(const Rec& x) {
  if constexpr (pair_clipped<Rec>) return (long long)x.t_end + (long long)x.clip_right;
  else return (long long)x.t_end;
}

// rec(t): the record awry_get_seq_location returns (a caller's position past the text: the last record, as map_select_kernel has it)
__device__ __forceinline__ uint64_t pair_record(const DevIndex& ix, uint64_t t) {
  uint64_t out[2];
  localise(ix, t < ix.bwt_len ? t : ix.bwt_len - 1, out);
  return out[0];
}

// proper(x, y): symmetric in its arguments -- f is the one on strand 0, v the one on strand 1.  The record search comes last.
// The order conditions are on the aligned spans in either mode; the insert is ve(v) - fb(f).
template <class Rec>
__device__ __forceinline__ bool pair_proper(const DevIndex& ix, const Rec& x, const Rec& y, uint32_t min_insert, uint32_t max_insert) {
  if ((x.strand != 0) == (y.strand != 0)) return false;
  const Rec& f = x.strand == 0 ? x : y;
  const Rec& v = x.strand == 0 ? y : x;
  if (f.t_begin > v.t_begin || f.t_end > v.t_end) return false;
  const long long ins = pair_ve(v) - pair_fb(f);
  if (ins < (long long)min_insert || ins > (long long)max_insert) return false;
  return pair_record(ix, f.t_begin) == pair_record(ix, v.t_begin);
}

template <class Rec> __device__ __forceinline__ bool pair_spans_intersect(const Rec& a, const Rec& b) {
  return a.strand == b.strand && (a.t_begin > b.t_begin ? a.t_begin : b.t_begin) < (a.t_end < b.t_end ? a.t_end : b.t_end);
}

// One slot per lane, grid-stride: slot w = (2p + m) G + a is candidate a of mate m of pair p.  The length of read i is
// qoff[qstride i + 1] - qoff[qstride i]: qstride 1 over the reads' own offsets, 2 over the doubled batch's.  An anchor writes the
// doubled-batch query it seeks, 4p + 2 (1 - m) + (1 - strand), and its window of starts cut to the text and to the record of its
// t_begin; every other slot, and an anchor whose window is empty, gets win_count = 0 and win_first = 0, and a slot that is no anchor
// names query 4p + 2 (1 - m), which exists, so that whoever reads the slot's query reads inside the batch.
// Rec = MapClipRec: the clipped mode's windows, measured from fb(x) and ve(x); a forward anchor's window still begins no earlier
// than its aligned span does.  With clips 0 they are the end-to-end windows.
template <class Rec>
__global__ __launch_bounds__(256) void pair_windows_kernel(DevIndex ix, const uint64_t* __restrict__ cand_off, const Rec* __restrict__ cands,
                                                           const uint64_t* __restrict__ qoff, uint32_t qstride, uint64_t P, PairParams pp,
                                                           uint32_t* __restrict__ win_query, uint64_t* __restrict__ win_first,
                                                           uint32_t* __restrict__ win_count) {
  const uint64_t G = pp.rescue_anchors, slots = 2 * P * G, stride = (uint64_t)gridDim.x * blockDim.x;
  const long long n_text = (long long)ix.bwt_len - 1, k = pp.rescue_edits, mn = pp.min_insert, mx = pp.max_insert;
  for (uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; w < slots; w += stride) {
    const uint64_t read = w / G, a = w - read * G, mate = read ^ 1ull;
    const uint64_t lo_m = cand_off[read], n_m = cand_off[read + 1] - lo_m, lo_o = cand_off[mate], n_o = cand_off[mate + 1] - lo_o;
    const uint64_t qb = qoff[(uint64_t)qstride * mate], qe = qoff[(uint64_t)qstride * mate + 1];
    const long long L = qe > qb ? (long long)(qe - qb) : 0;  // the other mate's length
    uint32_t query = (uint32_t)(2 * mate), count = 0;
    uint64_t first = 0;
    if (a < n_m && L > k && L <= (long long)EDIT_MAX_LEN) {
      const Rec x = cands[lo_m + a];
      bool paired = false;
      for (uint64_t j = 0; j < n_o && !paired; j++) paired = pair_proper(ix, x, cands[lo_o + j], pp.min_insert, pp.max_insert);
      if (!paired) {
        query = (uint32_t)(2 * mate) + (x.strand == 0 ? 1u : 0u);
        const long long tb = (long long)x.t_begin, fb = pair_fb(x), ve = pair_ve(x);
        long long lo, hi;
        if (x.strand == 0) {
          lo = tb + (fb - tb + mn - L - k > 0 ? fb - tb + mn - L - k : 0);  // max(t_begin, fb + min_insert - L' - k)
          hi = fb + mx - L + k;
        } else {
          lo = ve - mx;
          hi = tb < ve - mn ? tb : ve - mn;
        }
        uint64_t rec[2];
        localise(ix, x.t_begin < ix.bwt_len ? x.t_begin : ix.bwt_len - 1, rec);
        const long long r_lo = ix.nseq ? (long long)ix.seq_starts[rec[0]] : 0;
        const long long r_hi = rec[0] + 1 < ix.nseq ? (long long)ix.seq_starts[rec[0] + 1] : n_text;  // exclusive
        if (lo < r_lo) lo = r_lo;
        if (lo < 0) lo = 0;
        if (hi > r_hi - 1) hi = r_hi - 1;
        if (hi > n_text - 1) hi = n_text - 1;
        if (hi >= lo) { first = (uint64_t)lo; count = (uint32_t)(hi - lo + 1); }
      }
    }
    win_query[w] = query;
    win_first[w] = first;
    win_count[w] = count;
  }
}

// A window of more than `sub` starts as ceil(count / sub) windows of the same query, back to back: the scan runs one window per
// lane, and the hit rule of a start does not depend on which window owns it.  FILL = false: n_sub[w].  FILL = true: the pieces of
// window w at [sub_off[w], sub_off[w + 1]), in ascending position, so that the hits of window w are the hits of its pieces in order.
template <bool FILL>
__global__ __launch_bounds__(256) void pair_sub_windows_kernel(const uint32_t* __restrict__ win_query, const uint64_t* __restrict__ win_first,
                                                               const uint32_t* __restrict__ win_count, uint64_t m, uint32_t sub, uint64_t* __restrict__ n_sub,
                                                               const uint64_t* __restrict__ sub_off, uint32_t* __restrict__ sub_query,
                                                               uint64_t* __restrict__ sub_first, uint32_t* __restrict__ sub_count) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; w < m; w += stride) {
    const uint32_t cnt = win_count[w], pieces = cnt / sub + (cnt % sub ? 1u : 0u);
    if (!FILL) { n_sub[w] = pieces; continue; }
    const uint64_t out = sub_off[w], cap = sub_off[w + 1] - out, first = win_first[w];
    const uint32_t q = win_query[w];
    for (uint32_t j = 0; j < pieces && j < cap; j++) {
      sub_query[out + j] = q;
      sub_first[out + j] = first + (uint64_t)j * sub;
      sub_count[out + j] = cnt - j * sub < sub ? cnt - j * sub : sub;
    }
  }
}

// One window per lane: the hit with the smallest (distance, position) among the scan's fill output for the window's pieces
// [sub_off[w], sub_off[w + 1]) (sub_off == nullptr: the window is its own piece).  Hits lie in ascending position, so the first of
// the smallest distance is taken.  No hit: best_edits = PAIR_NO_HIT, best_gpos = 0.
__global__ __launch_bounds__(256) void pair_best_hit_kernel(const uint64_t* __restrict__ sub_off, const uint64_t* __restrict__ hit_off,
                                                            const uint64_t* __restrict__ gpos, const uint8_t* __restrict__ edits, uint64_t m,
                                                            uint64_t* __restrict__ best_gpos, uint8_t* __restrict__ best_edits) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; w < m; w += stride) {
    const uint64_t a = hit_off[sub_off ? sub_off[w] : w], z = hit_off[sub_off ? sub_off[w + 1] : w + 1];
    uint8_t e = PAIR_NO_HIT;
    uint64_t g = 0;
    for (uint64_t h = a; h < z; h++)
      if (edits[h] < e) { e = edits[h]; g = gpos[h]; }
    best_gpos[w] = g;
    best_edits[w] = e;
  }
}

// slot w's rescued candidate out of its best hit and the aligner's text_len; a slot without a hit (or whose triple the aligner did
// not take) holds edits = PAIR_NO_RESCUE.  Rec = MapClipRec: the candidate also carries score = a #'=' - b #'X' - g (#'I' + #'D')
// over its runs ops[w ALIGN_MAX_OPS ..) (length << 4 | BAM op) and clips 0, and exists only if score >= md.min_score.
template <class Rec>
__global__ __launch_bounds__(256) void pair_rescued_kernel(const uint32_t* __restrict__ win_query, const uint64_t* __restrict__ best_gpos,
                                                           const uint8_t* __restrict__ best_edits, const uint32_t* __restrict__ text_len,
                                                           const uint8_t* __restrict__ n_ops, uint64_t m, Rec* __restrict__ resc,
                                                           const uint32_t* __restrict__ ops, PairMode md) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; w < m; w += stride) {
    const bool ok = best_edits[w] != PAIR_NO_HIT && n_ops[w] != 0;
    const uint64_t g = best_gpos[w];
    if constexpr (pair_clipped<Rec>) {
      int score = 0;
      const uint32_t nr = ok ? (n_ops[w] < ALIGN_MAX_OPS ? n_ops[w] : ALIGN_MAX_OPS) : 0u;
      for (uint32_t i = 0; i < nr; i++) {
        const uint32_t run = ops[w * ALIGN_MAX_OPS + i];
        const int len = (int)(run >> 4), op = (int)(run & 15u);
        score += len * (op == 7 ? md.match : op == 8 ? -md.mismatch : -md.gap);
      }
      resc[w] = ok && score >= md.min_score
                    ? Rec{g, g + text_len[w], best_edits[w], 0u, PAIR_NO_CHAIN, (uint8_t)(win_query[w] & 1u), (uint8_t)0, MAP_RESCUED, score, (uint16_t)0, (uint16_t)0}
                    : Rec{0, 0, PAIR_NO_RESCUE, 0u, PAIR_NO_CHAIN, (uint8_t)0, (uint8_t)0, (uint16_t)0, 0, (uint16_t)0, (uint16_t)0};
    } else {
      resc[w] = ok ? MapRec{g, g + text_len[w], best_edits[w], 0u, PAIR_NO_CHAIN, (uint8_t)(win_query[w] & 1u), (uint8_t)0, MAP_RESCUED}
                   : MapRec{0, 0, PAIR_NO_RESCUE, 0u, PAIR_NO_CHAIN, (uint8_t)0, (uint8_t)0, (uint16_t)0};
    }
  }
}

// the index of the i-th set bit of mask (i < popcount)
__device__ __forceinline__ uint32_t pair_nth_bit(uint32_t mask, uint32_t i) {
  while (i--) mask &= mask - 1;
  return (uint32_t)__ffs((int)mask) - 1u;
}

// One pair per lane, grid-stride.  K'_t is K_t = cands[cand_off[2p + t] ..) followed by the rescued candidates aimed at mate t --
// slots ((2p + 1 - t) G + a), a ascending -- each unless its span intersects that of a same-strand member already there; which
// slots are appended is a G-bit mask, and every record is re-read where it is needed: no array lives in registers.  The pairs of
// K'_0 x K'_1 are walked in index order, so a strictly smaller (cost, improper) replaces the best and ties stay with the earlier
// pair; the second pair's cost is the smallest among the others.  resc == nullptr: no rescue (G = 0).
// FILL = false: n_maps[2p], n_maps[2p + 1].  FILL = true: the records at maps[map_off[i]] (never a slot at or beyond map_off[i + 1]),
// per record (both nullable) sel = the index into cands or PAIR_SEL_RESCUED | slot, pos = record and offset of t_begin; insert[p]
// (nullable).
// Rec = MapClipRec: the clipped mode of the same choice: cost = -(x.score + y.score) + (U if improper), signed, so the order is
// ascending by (-S, !proper, i, j); MAPQ is min(60, 10 (S1 - S2) / md.mapq_div); the insert is ve(v) - fb(f).
template <bool FILL, class Rec>
__global__ __launch_bounds__(256) void pair_select_kernel(DevIndex ix, const uint64_t* __restrict__ cand_off, const Rec* __restrict__ cands,
                                                          const Rec* __restrict__ resc, const uint8_t* __restrict__ read_status, uint64_t P, PairParams pp,
                                                          uint64_t* __restrict__ n_maps, const uint64_t* __restrict__ map_off, Rec* __restrict__ maps,
                                                          uint32_t* __restrict__ sel, uint64_t* __restrict__ pos, uint32_t* __restrict__ insert, PairMode md) {
  constexpr bool CLIP = pair_clipped<Rec>;
  using Cost = std::conditional_t<CLIP, int32_t, uint32_t>;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  const uint32_t G = resc ? pp.rescue_anchors : 0u, U = pp.unpaired_penalty;
  for (uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; p < P; p += stride) {
    const uint64_t lo0 = cand_off[2 * p], lo1 = cand_off[2 * p + 1], hi1 = cand_off[2 * p + 2];
    const uint32_t n0 = (uint32_t)(lo1 - lo0), n1 = (uint32_t)(hi1 - lo1);
    auto base_of = [&](uint32_t t) { return (2 * p + 1 - t) * (uint64_t)G; };  // the first slot whose rescued candidate is aimed at mate t
    auto appended = [&](uint32_t t) {
      const uint64_t lo = t ? lo1 : lo0, base = base_of(t);
      const uint32_t n = t ? n1 : n0;
      uint32_t acc = 0;
      for (uint32_t a = 0; a < G; a++) {
        const Rec z = resc[base + a];
        if (z.edits == PAIR_NO_RESCUE) continue;
        bool redundant = false;
        if (FILL) {  // (the count pass asks only whether a list is empty, and a first member is never dropped)
          for (uint32_t j = 0; j < n; j++) redundant |= pair_spans_intersect(z, cands[lo + j]);
          for (uint32_t m = acc; m; m &= m - 1) redundant |= pair_spans_intersect(z, resc[base + (uint32_t)__ffs((int)m) - 1u]);
        }
        if (!redundant) acc |= 1u << a;
      }
      return acc;
    };
    const uint32_t acc0 = appended(0), acc1 = appended(1);
    const uint32_t c0 = n0 + (uint32_t)__popc(acc0), c1 = n1 + (uint32_t)__popc(acc1);
    if (!FILL) {
      n_maps[2 * p] = c0 ? 1 : 0;
      n_maps[2 * p + 1] = c1 ? 1 : 0;
      continue;
    }
    // member i of K'_t as an index into cands, or PAIR_SEL_RESCUED | slot
    auto where = [&](uint32_t t, uint32_t i) -> uint32_t {
      const uint32_t n = t ? n1 : n0;
      if (i < n) return (uint32_t)((t ? lo1 : lo0) + i);
      return PAIR_SEL_RESCUED | (uint32_t)(base_of(t) + pair_nth_bit(t ? acc1 : acc0, i - n));
    };
    auto get = [&](uint32_t at) { return at & PAIR_SEL_RESCUED ? resc[at & ~PAIR_SEL_RESCUED] : cands[at]; };
    auto emit = [&](uint64_t read, uint32_t at, const Rec& rec) {
      const uint64_t out = map_off[read];
      if (map_off[read + 1] <= out) return;
      maps[out] = rec;
      if (sel) sel[out] = at;
      if (pos) localise(ix, rec.t_begin < ix.bwt_len ? rec.t_begin : ix.bwt_len - 1, pos + 2 * out);
    };
    uint32_t ins = 0;
    if (c0 && c1) {
      Cost best_cost = 0, second_cost = 0;
      uint32_t best_x = 0, best_y = 0;
      bool best_proper = false, have = false, have2 = false;
      for (uint32_t i = 0; i < c0; i++) {
        const Rec x = get(where(0, i));
        for (uint32_t j = 0; j < c1; j++) {
          const Rec y = get(where(1, j));
          const bool pr = pair_proper(ix, x, y, pp.min_insert, pp.max_insert);
          Cost cost;
          if constexpr (CLIP) cost = -(x.score + y.score) + (pr ? 0 : (int32_t)U);
          else cost = x.edits + y.edits + (pr ? 0u : U);
          if (!have || cost < best_cost || (cost == best_cost && pr && !best_proper)) {
            if (have) { second_cost = best_cost; have2 = true; }  // (the old best is no worse than any other seen so far)
            best_cost = cost; best_proper = pr; best_x = i; best_y = j; have = true;
          } else if (!have2 || cost < second_cost) {
            second_cost = cost; have2 = true;
          }
        }
      }
      const bool capped = read_status && (read_status[2 * p] == Q_SEED_CAP || read_status[2 * p + 1] == Q_SEED_CAP);
      uint32_t q10;  // ten times the gap between the best and the second pair (>= 0: the order), CLIP: in units of a + b, rounded down
      if constexpr (CLIP) q10 = have2 ? (uint32_t)(10 * ((int64_t)second_cost - (int64_t)best_cost) / (int64_t)md.mapq_div) : 0u;
      else q10 = 10u * (have2 ? second_cost - best_cost : 0u);
      const uint8_t mapq = (uint8_t)(capped ? 0u : !have2 ? MAP_MAPQ_MAX : (q10 < MAP_MAPQ_MAX ? q10 : MAP_MAPQ_MAX));
      const uint32_t ax = where(0, best_x), ay = where(1, best_y);
      Rec x = get(ax), y = get(ay);
      if (best_proper) ins = (uint32_t)((x.strand == 0 ? pair_ve(y) : pair_ve(x)) - (x.strand == 0 ? pair_fb(x) : pair_fb(y)));
      x.mapq = y.mapq = mapq;
      x.flags = (uint16_t)((x.flags & MAP_RESCUED) | (best_proper ? MAP_PROPER_PAIR : 0));
      y.flags = (uint16_t)((y.flags & MAP_RESCUED) | (best_proper ? MAP_PROPER_PAIR : 0));
      emit(2 * p, ax, x);
      emit(2 * p + 1, ay, y);
    } else if (c0 || c1) {  // one mate alone: its single-end primary, as map_select_kernel wrote it
      const uint32_t t = c0 ? 0u : 1u, at = where(t, 0);
      Rec x = get(at);
      x.flags = (uint16_t)(x.flags | MAP_MATE_UNMAPPED);
      emit(2 * p + t, at, x);
    }
    if (insert) insert[p] = ins;
  }
}

}  // namespace awry
