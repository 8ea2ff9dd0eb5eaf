// kernels_map.hip.h -- map reads on both strands: the doubled batch (every read as given and reverse-complemented), the ranking of
// a read's aligned chains of both strands, the redundancy rule, MAPQ, and the gather of the reported alignments for the CIGAR
// fill pass.  Included by kernels.hip.h after kernels_chain_align.hip.h (it uses Aln, Chain, Seed, localise, the alphabet maps).
//
// No counterpart in the reference.  The definition is the one include/awry_hip.h states ("map reads on both strands"); in short,
// for read i the candidates are the alignments with status AWRY_ALN_OK among the first chains_per_strand chains of query 2i
// (strand 0) and of query 2i + 1 (strand 1, the reverse complement), ranked ascending by (edits, -chain score, strand, t_begin,
// chain index); a candidate is dropped when a better-ranked kept one of its strand has an intersecting text span; the first
// max_report kept ones are the read's records.
#pragma once

namespace awry {

constexpr int MAP_MAX_CHAINS = 8;          // AWRY_MAP_MAX_CHAINS: chains per strand that can become candidates
constexpr uint16_t MAP_SECONDARY = 1;      // AWRY_MAP_SECONDARY
constexpr uint32_t MAP_MAPQ_MAX = 60;
constexpr int MAP_EXPAND_GROUP = 16;       // lanes that own a read in strand_expand_kernel

struct MapRec {  // == awry_map_t (checked in map_host.h)
  uint64_t t_begin, t_end;
  uint32_t edits, chain_score, chain_index;
  uint8_t strand, mapq;
  uint16_t flags;
};

// The doubled batch: query 2i = read i as given, query 2i + 1 = rc(read i); out_off[2i] = 2 (off[i] - off[0]), out_off[2i + 1] =
// that + L_i, out_off[2n] = 2 (off[n] - off[0]).  A group of MAP_EXPAND_GROUP lanes owns a read and walks it 16 bytes at a time:
// lane l loads byte x + l, stores it at the same place of the copy and its complement at the mirrored place of the reverse
// strand, so the loads and both stores of a group are one contiguous span each.  Nothing is written past out_bytes[2 (off[n] -
// off[0])) or out_off[2n].
__global__ __launch_bounds__(256) void strand_expand_kernel(const uint8_t* __restrict__ bytes, const uint64_t* __restrict__ off, uint64_t n,
                                                            uint8_t* __restrict__ out_bytes, uint64_t* __restrict__ out_off) {
  constexpr int G = MAP_EXPAND_GROUP;
  const uint64_t groups = (uint64_t)gridDim.x * (blockDim.x / G);
  const uint32_t l = threadIdx.x % G;
  const uint64_t base = n ? off[0] : 0;
  for (uint64_t i = (uint64_t)blockIdx.x * (blockDim.x / G) + threadIdx.x / G; i < n; i += groups) {
    const uint64_t b = off[i], e = off[i + 1];
    const uint64_t L = e > b ? e - b : 0, to = 2 * (b - base);
    if (l == 0) {
      out_off[2 * i] = to;
      out_off[2 * i + 1] = to + L;
      if (i + 1 == n) out_off[2 * n] = to + 2 * L;
    }
    for (uint64_t x = l; x < L; x += G) {
      const uint8_t a = bytes[b + x];
      out_bytes[to + x] = a;
      out_bytes[to + L + (L - 1 - x)] = nt_complement_ascii(a);
    }
  }
}

struct MapClipRec {  // == awry_map_clip_t (checked in map_host.h): MapRec's fields, then the alignment's score and clips
  uint64_t t_begin, t_end;
  uint32_t edits, chain_score, chain_index;
  uint8_t strand, mapq;
  uint16_t flags;
  int32_t score;
  uint16_t clip_left, clip_right;
};
template <bool CLIP> using MapRecOf = std::conditional_t<CLIP, MapClipRec, MapRec>;

// The mode of a selection: end to end (the default), or over clipped records with the score threshold T and the MAPQ divisor a + b.
struct MapMode { bool clip = false; int min_score = 0, mapq_div = 1; };

// the rank key of a candidate, ascending (k0, k1, strand, t_begin, j): (edits, -chain score) end to end, (-score, edits) clipped
struct MapKey {
  int64_t k0, k1;
  uint32_t strand, j;
  uint64_t t_begin;
  __device__ __forceinline__ bool before(const MapKey& o) const {
    if (k0 != o.k0) return k0 < o.k0;
    if (k1 != o.k1) return k1 < o.k1;
    if (strand != o.strand) return strand < o.strand;
    if (t_begin != o.t_begin) return t_begin < o.t_begin;
    return j < o.j;
  }
};
template <bool CLIP> __device__ __forceinline__ MapKey map_key(const AlnOf<CLIP>& a, uint32_t chain_score, uint32_t c) {
  if constexpr (CLIP) return MapKey{-(int64_t)a.score, (int64_t)a.edits, c >> 3, c & 7u, a.t_begin};
  else return MapKey{(int64_t)a.edits, -(int64_t)chain_score, c >> 3, c & 7u, a.t_begin};
}

// One read per lane, grid-stride.  The candidates of read i are slots c = 8 s + j, j < min(aln_off[2i + s + 1] - aln_off[2i + s],
// A), of alignment aln_off[2i + s] + j.  They are ranked by selection: each round takes the smallest key among the slots not yet
// taken (a 16-bit mask; the records are re-read, no array lives in registers), keeps it unless a kept slot of its strand has an
// intersecting span (max(b1, b2) < min(e1, e2); an empty span intersects nothing), and stops when nothing is left or enough is
// kept: R in the count pass, max(R, 2) in the fill pass, which needs the second kept candidate's edits for MAPQ.
// FILL = false: n_maps[i] = min(R, kept) and read_status[i] (nullable) = Q_SEED_CAP if either strand's chain status is, else Q_OK.
// FILL = true: the records at maps[map_off[i] ..), and per record (both nullable) sel[k] = the alignment's index and pos[2k ..] =
// record and offset of t_begin; never a slot at or beyond map_off[i + 1].
// CLIP = true: the clipped mode of the same selection (include/awry_hip.h, "soft-clip read ends") over awry_aln_clip_t records: a
// candidate also needs score >= md.min_score, the key is (-score, edits, ..), MAPQ is min(60, 10 (s1 - s2) / md.mapq_div), and the
// records are awry_map_clip_t.
template <bool FILL, bool CLIP>
__global__ __launch_bounds__(256) void map_select_kernel(DevIndex ix, const uint64_t* __restrict__ aln_off, const AlnOf<CLIP>* __restrict__ alns,
                                                         const Chain* __restrict__ chains, const uint8_t* __restrict__ chain_status, uint64_t n, uint32_t A,
                                                         uint32_t R, uint64_t* __restrict__ n_maps, uint8_t* __restrict__ read_status,
                                                         const uint64_t* __restrict__ map_off, MapRecOf<CLIP>* __restrict__ maps, uint32_t* __restrict__ sel,
                                                         uint64_t* __restrict__ pos, MapMode md) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const uint64_t lo0 = aln_off[2 * i], lo1 = aln_off[2 * i + 1], hi1 = aln_off[2 * i + 2];
    const uint32_t c0 = (uint32_t)(lo1 - lo0 < A ? lo1 - lo0 : A), c1 = (uint32_t)(hi1 - lo1 < A ? hi1 - lo1 : A);
    const bool capped = chain_status && (chain_status[2 * i] == Q_SEED_CAP || chain_status[2 * i + 1] == Q_SEED_CAP);
    auto at = [&](uint32_t c) { return (c >> 3 ? lo1 : lo0) + (c & 7u); };
    uint32_t open = 0;  // candidate slots not yet taken
    auto candidate = [&](uint64_t a) {
      if constexpr (CLIP) return alns[a].status == ALN_OK && alns[a].score >= md.min_score;
      else return alns[a].status == ALN_OK;
    };
    for (uint32_t j = 0; j < c0; j++) open |= candidate(lo0 + j) ? 1u << j : 0u;
    for (uint32_t j = 0; j < c1; j++) open |= candidate(lo1 + j) ? 1u << (8 + j) : 0u;
    const uint32_t need = FILL ? (R > 2u ? R : 2u) : R;
    const uint64_t out = FILL ? map_off[i] : 0, cap = FILL ? map_off[i + 1] - out : 0;
    uint32_t kept = 0, nkept = 0;
    int64_t first_k0 = 0, second_k0 = 0;  // k0 of the first and second kept candidates: their edits, CLIP: minus their scores
    while (open && nkept < need) {
      uint32_t best = 0;
      MapKey bk{};
      bool have = false;
      for (uint32_t m = open; m; m &= m - 1) {
        const uint32_t c = (uint32_t)__ffs((int)m) - 1u;
        const uint64_t a = at(c);
        const MapKey k = map_key<CLIP>(alns[a], chains[a].score, c);
        if (!have || k.before(bk)) { bk = k; best = c; have = true; }
      }
      open &= ~(1u << best);
      const uint64_t b1 = bk.t_begin, e1 = alns[at(best)].t_end;
      bool redundant = false;
      for (uint32_t m = kept & (best >> 3 ? 0xFF00u : 0x00FFu); m; m &= m - 1) {
        const AlnOf<CLIP> o = alns[at((uint32_t)__ffs((int)m) - 1u)];
        redundant |= (b1 > o.t_begin ? b1 : o.t_begin) < (e1 < o.t_end ? e1 : o.t_end);
      }
      if (redundant) continue;
      kept |= 1u << best;
      if (nkept == 0) first_k0 = bk.k0;
      if (nkept == 1) second_k0 = bk.k0;
      if (FILL && nkept < R && nkept < cap) {  // (the primary's mapq is settled below, once the second kept candidate is known)
        const AlnOf<CLIP> w = alns[at(best)];
        const uint32_t cs = chains[at(best)].score;
        const uint16_t fl = (uint16_t)(nkept ? MAP_SECONDARY : 0);
        if constexpr (CLIP) maps[out + nkept] = MapClipRec{b1, e1, w.edits, cs, bk.j, (uint8_t)bk.strand, (uint8_t)0, fl, w.score, w.clip_left, w.clip_right};
        else maps[out + nkept] = MapRec{b1, e1, w.edits, cs, bk.j, (uint8_t)bk.strand, (uint8_t)0, fl};
        if (sel) sel[out + nkept] = (uint32_t)at(best);
        if (pos) localise(ix, b1 < ix.bwt_len ? b1 : ix.bwt_len - 1, pos + 2 * (out + nkept));  // (a caller's record past the text: the last record)
      }
      nkept++;
    }
    if (FILL) {
      if (nkept && cap) {
        const int64_t d = nkept > 1 ? 10 * (second_k0 - first_k0) / (CLIP ? (int64_t)md.mapq_div : 1) : 0;  // (>= 0: the rank order)
        maps[out].mapq = (uint8_t)(capped ? 0u : nkept < 2 ? MAP_MAPQ_MAX : (d < (int64_t)MAP_MAPQ_MAX ? (uint32_t)d : MAP_MAPQ_MAX));
      }
    } else {
      n_maps[i] = nkept < R ? nkept : R;
      if (read_status) read_status[i] = capped ? Q_SEED_CAP : Q_OK;
    }
  }
}

// The reported alignments as a chain list of their own, for launch_chain_align's fill pass.  Pass 1 (win_members == nullptr), one
// record per lane: win_query[k] = chain_query[sel[k]], win_mcnt[k] = the members of alignment sel[k], win_nops[k] = n_ops[sel[k]]
// (both scan inputs).  Pass 2: the members of alignment sel[k] copied to win_members[win_moff[k] ..).
__global__ __launch_bounds__(256) void map_gather_kernel(const uint32_t* __restrict__ sel, uint64_t m, const uint32_t* __restrict__ chain_query,
                                                         const uint64_t* __restrict__ member_off, const Seed* __restrict__ members,
                                                         const uint64_t* __restrict__ n_ops, uint32_t* __restrict__ win_query, uint64_t* __restrict__ win_mcnt,
                                                         uint64_t* __restrict__ win_nops, const uint64_t* __restrict__ win_moff,
                                                         Seed* __restrict__ win_members) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < m; k += stride) {
    const uint64_t a = sel[k], from = member_off[a], cnt = member_off[a + 1] - from;
    if (!win_members) {
      win_query[k] = chain_query[a];
      win_mcnt[k] = cnt;
      win_nops[k] = n_ops[a];
      continue;
    }
    const uint64_t to = win_moff[k];
    for (uint64_t x = 0; x < cnt; x++) win_members[to + x] = members[from + x];
  }
}

}  // namespace awry
