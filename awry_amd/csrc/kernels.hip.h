// kernels.hip.h -- gfx950 (CDNA4, wave64) kernels of the FM-index hot path.  The umbrella header: the kernels live in the
// parts included below, one per kernel family, in dependency order; the locate family is still here, behind them.
//
//   rank / Occ        /root/reference src/bwt.rs:114-135,230-271 + src/simd_instructions.rs:96-121
//   step              src/fm_index.rs:559-582 (update_range_with_symbol)
//   backward search   src/fm_index.rs:402-438 + src/kmer_lookup_table.rs:90-110
//   backtrace/locate  src/fm_index.rs:516-544,585-593 + src/compressed_suffix_array.rs:76-111
//   localisation      src/sequence_index.rs:108-141 (intended semantics)
//
// Integer/bit path only (no MFMA): every kernel is bound by random 128-B line fetches from HBM.
// Two families:
//   * "scalar" kernels: one query (or one hit) per lane, any alphabet, any symbol, any length;
//   * "quad" kernels: the hot count path for packed nucleotide k-mers.  A wavefront holds 16
//     independent queries, one per QUAD of lanes; a quad fetches a 128-B block as 2 x
//     global_load_dwordx4 per lane (4 lanes x 16 B = one 64-B half line per instruction), ranks its
//     64-symbol slice with __popcll and sums partials with two quad_perm DPP adds -- no LDS round trip.
//
// Kernel map (default in CAPS; the others are kept as measured alternatives; [part] = the file):
//   count, any query      COUNT_SCALAR_KERNEL<A>             ASCII + offsets, one query per lane, seed probe, verify against text8 [kernels_count]
//   count, amino k-mers   COUNT_AA_KMER_PROBE_KERNEL         equal-length ASCII residues, one query per lane: entry / text decide most [kernels_aa_kmer]
//                         + COUNT_SCALAR_KERNEL<AMINO, LIST> the generic kernel on the listed rest [kernels_count]
//   count, packed k-mers  COUNT_NT2_PROBE_KERNEL             phase 1: one query per lane, entry / context / text decide most [kernels_nt2_kmer]
//                         + COUNT_NT2_RESUME_KERNEL          phase 2: quads resume the listed survivors (sparse seed tables) [kernels_nt2_kmer]
//                         COUNT_NT2_QUAD4_KERNEL             groups of four queries per quad (dense seed tables) [kernels_nt2_kmer]
//                         count_nt2_quad_kernel              one strided query per quad [kernels_nt2_kmer]
//                         count_nt2_chunk_kernel             queries/results staged through LDS per wave [kernels_nt2_kmer]
//   count, packed reads   COUNT_NT2_READS_PROBE_KERNEL<R>    phase 1 for reads of any (per-read) length [kernels_reads]
//                         + COUNT_NT2_READS_KERNEL<..LIST>   quads on the listed reads; without LIST: the single-kernel schedule [kernels_reads]
//                         + LCX_QUAD_READS_KERNEL<R>         the listed reads as one pool, when the left-context index is resident [lcx_kernels]
//   anchors, any query    ANCHOR_SCALAR_KERNEL<A, FILL>      greedy longest-match factorisation, one query per lane: count pass, scan, fill pass [kernels_anchor]
//                         + ANCHOR_RANGES_KERNEL             anchor records -> row pairs and located counts for the locate kernels [kernels_anchor]
//   SMEMs, any query      SMEM_SCALAR_KERNEL<A, FWD, FILL>   all super-maximal exact matches, one query per lane: forward extension by a search of
//                                                            the dense SA against text8 (FWD = SA) or by bisection over backward searches (FWD = LF),
//                                                            then the anchor walk; count pass, scan, fill pass, ANCHOR_RANGES_KERNEL [kernels_smem]
//   locate within k edits EDIT_SCAN_KERNEL<A, W, FILL>       Myers / Hyyro bit-vector scan of text windows, one window per lane, W = 1..4 words of
//                                                            64 query letters: count pass, scan, fill pass [edit_kernels]
//                         + EDIT_MASKS_KERNEL<A>             pattern masks of the queries, into the stream's workspace [edit_kernels]
//                         + edit_cap / diagonals / run_heads / run_ends / windows / query_hit_off / localise kernels: located pieces ->
//                                                            sorted diagonals -> windows, and the hits' records [edit_kernels]
//   align edit hits       EDIT_ALIGN_KERNEL<A, H>          banded table (half-width H = 2, 4, 6, 8 in registers) with a traceback through per-row
//                                                            direction words in a lane-interleaved workspace, one hit per lane: text span and
//                                                            CIGAR runs at a fixed stride [kernels_align]
//                         + align_hit_query / counts / compact kernels: the hits' queries, and fixed stride -> CSR [kernels_align]
//   chain located seeds   CHAIN_KERNEL<G, FILL>              sort, windowed dynamic programme and backtrack, one query per group of G = 64 or 16
//                                                            lanes, lane l on predecessor i - 1 - l, DPP maximum: count pass, two scans, fill
//                                                            pass [kernels_chain]
//                         + chain_expand / chain_seed_off kernels: located SMEM records -> seeds and per-query seed offsets [kernels_chain]
//   align chains          CHAIN_ALIGN_KERNEL<A, NBMAX, FILL> pieces as diagonal runs, banded tables (NBMAX = 9, 17, 33 cells in registers) for the
//                                                            extensions and gaps, one CIGAR per chain; one chain per lane over a class list, two
//                                                            passes [kernels_chain_align]
//                         + chain_align_classify / take / select / gather kernels: class lists, and the first chains of each query [kernels_chain_align]
//   map both strands      STRAND_EXPAND_KERNEL               reads -> the doubled batch (read, reverse complement), 16 lanes per read [kernels_map]
//                         + MAP_SELECT_KERNEL<FILL>          one read per lane: rank the aligned chains of both strands by selection, drop
//                                                            redundant spans, MAPQ; count pass, scan, fill pass [kernels_map]
//                         + MAP_GATHER_KERNEL                the reported alignments as a chain list for the CIGAR fill pass [kernels_map]
//   split reads           MAP_SPLIT_SELECT_KERNEL<FILL>      one read per lane: the clipped candidates walked in rank order by query interval --
//                                                            segments (primary, supplementaries), their secondaries, a MAPQ per segment;
//                                                            classify, then emit; count pass, scan, fill pass [kernels_split]
//   map read pairs        PAIR_WINDOWS_KERNEL<Rec>           one candidate slot per lane: is it an anchor, and the window of starts in which it
//                                                            expects the other mate [kernels_pair]
//                         + pair_sub_windows / PAIR_BEST_HIT / PAIR_RESCUED<Rec> kernels: windows cut for the edit scan, the smallest (distance,
//                                                            position) hit of a window, the rescued candidate [kernels_pair]
//                         + PAIR_SELECT_KERNEL<FILL, Rec>    one pair per lane: rescued candidates appended, the pair of smallest cost, pair
//                                                            MAPQ, flags, insert; count pass, scan, fill pass [kernels_pair]
//                                                            (Rec = MapClipRec: the clipped mode -- inserts through the clips, pairs by score)
//   count, wide rows      count_nt2_wide_kernel, count_nt2_wide_probe_kernel   64-bit rows [kernels_wide]
//   locate                LOCATE_TILE_KERNEL<A>              hit -> row, sampled / verified hits finished [this file]
//                         + LOCATE_WALK_NT_LANE_KERNEL       LF walks of the rest, one hit per lane, whole block per step [this file]
//                         + LOCALISE_WALKED_KERNEL           record / offset of the walked hits [this file]
//                         LOCATE_WALK_KERNEL<AMINO>          generic walk, the amino indexes' second pass [this file]
//   accelerators          seed_level1/extend<Entry>, seed_finalize, seed64_finalize (+aa_seed_*), seed_rows_to_positions_kernel [kernels_seed];
//                         densify_sa_kernel, nblock_sa_kernel, text4_scatter_kernel, text8_scatter_kernel [this file];
//                         text8_chains_kernel (the text without the dense SA, for the edit scan) [edit_kernels];
//                         kt_scan_kernel<INSERT> (the k-mer count table of one query length, from the left-context index) [kmer_table]
//   glue                  pack_nt2_tile_kernel<R> [kernels_pack]; scan_*_kernel, stream_copy_kernel, phase_marker_kernel,
//                         narrow_counts_kernel, status_first_bad_kernel [kernels_scan]; ref_kmer_table_kernel, scalar_ops_kernel [kernels_count]
//   device helpers        scalar rank / step / backstep, ByteStream, text_equals_query [kernels_rank]; wave / block scans [kernels_scan];
//                         quad_sum / quad_load / quad_rank_part / quad_step<Row>, text windows, verify_part [kernels_quad];
//                         the left-context index's search and its construction kernels [lcx]
#pragma once
#include <hip/hip_runtime.h>

#include "alphabet.h"
#include "layout.h"

// each part needs the ones above it
#include "kernels_rank.hip.h"
#include "kernels_scan.hip.h"
#include "kernels_count.hip.h"     // block_excl_scan
#include "kernels_anchor.hip.h"    // step_scalar, ByteStream, seed_probe, tally_add
#include "kernels_smem.hip.h"      // Anchor, ascii_query_status, seed_rows_ending_at, nt_indices8
#include "kernels_aa_kmer.hip.h"   // QueryList, tally_add
#include "kernels_quad.hip.h"      // slice_mask
#include "lcx.hip.h"               // quad_sum, Text20
#include "kernels_nt2_kmer.hip.h"  // quad_step, verify_part, lcx_quad_step
#include "kmer_table.hip.h"        // lcx_text_letters, LCX_LANE_ROWS
#include "kernels_seed.hip.h"      // quad_step, step_scalar, symbol_at, Text20
#include "kernels_pack.hip.h"
#include "kernels_reads.hip.h"     // Nt2Survivors
#include "lcx_kernels.hip.h"       // Nt2Survivors, block_excl_scan, lcx_quad_step
#include "kernels_wide.hip.h"      // Nt2Survivors

namespace awry {

// ------------------------------------------------------------------------------------------------
// locate v2: tiles of hits, per-lane walk state machines, optional dense device SA
// ------------------------------------------------------------------------------------------------
constexpr int LOC_TILE = 1024;  // hits per tile (one 256-thread block at a time)
constexpr int LOC_QCAP = 1024;  // query (offset, start) pairs cached in LDS per tile

// value of the suffix array at a sampled row: the file's bit-packed samples (rows r % sa_ratio == 0) or the
// dense device array (rows r % dense_ratio == 0, u32 entries) built by densify_sa_kernel
constexpr uint64_t LOC_WALK_FLAG = 1ull << 63;  // gpos[h] holds a BWT row that still has to walk to a sampled row

// global text position -> (record, offset): largest i with seq_starts[i] <= g (the intended semantics of
// src/sequence_index.rs:108-141, see SURVEY a-17)
__device__ __forceinline__ void localise(const DevIndex& ix, uint64_t g, uint64_t* __restrict__ out) {
  uint64_t a = 0, z = ix.nseq;
  if (ix.seq_bucket) {  // the records of g's bucket: from the one holding the bucket's first position to the one holding the next bucket's
    const uint64_t b = g >> ix.seq_bucket_shift;
    a = ix.seq_bucket[b];
    z = (uint64_t)ix.seq_bucket[b + 1] + 1;
  }
  while (z - a > 1) { uint64_t mid = (a + z) >> 1; if (ix.seq_starts[mid] <= g) a = mid; else z = mid; }
  out[0] = a;
  out[1] = g - (ix.nseq ? ix.seq_starts[a] : 0);
}
// the same over a copy of the record starts in LDS (a block loads it once): the search is a chain of dependent loads
constexpr int LOC_SEQ_LDS = 1024;
__device__ __forceinline__ void localise_lds(const uint64_t* s_starts, uint64_t nseq, uint64_t g, uint64_t* __restrict__ out) {
  uint64_t a = 0, z = nseq;
  while (z - a > 1) { uint64_t mid = (a + z) >> 1; if (s_starts[mid] <= g) a = mid; else z = mid; }
  out[0] = a;
  out[1] = g - (nseq ? s_starts[a] : 0);
}

// row -> "is it a sampled row" / sample index, without a 64-bit division per backstep (the test runs once per LF step;
// a generic u64 modulo is ~100 instructions and made the walk ALU-bound): power-of-two ratios (the default 8) use a
// mask and a shift, other ratios a 32-bit division while the row fits.
__device__ __forceinline__ bool ratio_divides(uint64_t ratio, uint64_t row) {
  if ((ratio & (ratio - 1)) == 0) return (row & (ratio - 1)) == 0;
  if ((row >> 32) == 0 && (ratio >> 32) == 0) return (uint32_t)row % (uint32_t)ratio == 0u;
  return row % ratio == 0;
}
__device__ __forceinline__ uint64_t ratio_quotient(uint64_t ratio, uint64_t row) {
  if ((ratio & (ratio - 1)) == 0) return row >> (63 - __clzll((long long)ratio));
  if ((row >> 32) == 0 && (ratio >> 32) == 0) return (uint32_t)row / (uint32_t)ratio;
  return row / ratio;
}
__device__ __forceinline__ bool row_is_sampled(const DevIndex& ix, const uint32_t* dense, uint32_t dense_ratio, uint64_t row) {
  return ratio_divides(dense ? (uint64_t)dense_ratio : ix.sa_ratio, row);
}
__device__ __forceinline__ uint64_t row_sample(const DevIndex& ix, const uint32_t* dense, uint32_t dense_ratio, uint64_t row) {
  return dense ? (uint64_t)dense[ratio_quotient(dense_ratio, row)] : sa_sample(ix, ratio_quotient(ix.sa_ratio, row));
}
// (sample + steps) % bwt_len of src/fm_index.rs:534; sample < bwt_len and a walk is shorter than the text
__device__ __forceinline__ uint64_t walked_position(uint64_t sample, uint64_t steps, uint64_t bwt_len) {
  const uint64_t g = sample + steps;
  return g >= bwt_len ? g - bwt_len : g;
}

// dense[j] = SA[j * dense_ratio] for every j, recovered from the file's samples by CHAINS: the thread of sampled row
// s (SA known) walks LF -- visiting the rows of text positions SA[s]-1, SA[s]-2, ... -- and fills them in until it
// meets the next sampled row, where another thread's chain starts.  Every row is visited exactly once (n LF steps in
// total).  Walking from every unsampled row to its next sample instead costs the SUM of those distances, which is
// quadratic in the gap length, and row sampling leaves gaps of millions of rows inside long N runs (LF moves by a
// constant stride there): 121 s instead of 1 s on a chr1-scale text.
template <int A>
__global__ __launch_bounds__(256) void densify_sa_kernel(DevIndex ix, uint32_t dense_ratio, uint64_t nsamples, uint32_t* __restrict__ dense) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  const uint32_t fr = ix.sa_ratio;  // rows and SA values fit 32 bits here (the dense SA needs bwt_len < 2^32)
  for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < nsamples; j += stride) {
    uint32_t row = (uint32_t)(j * fr);
    uint32_t v = (uint32_t)sa_sample(ix, j);
    for (;;) {
      const uint32_t e = row / dense_ratio;
      if (e * dense_ratio == row) dense[e] = v;
      row = (uint32_t)backstep_scalar<A>(ix, row);
      if (row % fr == 0u) break;  // a sampled row: its own chain takes over
      v--;                        // the suffix one text position to the left (v > 0 here: only SA = 0 steps to row 0)
    }
  }
}

// the text as 4-bit codes, recovered from the index itself: T[SA[r] - 1] = BWT[r] (T[n-1] = '$' for the row with SA = 0).
// Needs the dense SA at ratio 1.  Codes: A0 C1 G2 T3, everything else has bit 3 set and never equals a query letter.
template <int A>
__global__ __launch_bounds__(256) void text4_scatter_kernel(DevIndex ix, uint32_t* __restrict__ text4) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < ix.bwt_len; r += stride) {
    const uint64_t v = ix.dense_sa[r];
    const uint64_t p = v ? v - 1 : ix.bwt_len - 1;
    const int letter = nt_letter_of_index(symbol_at<A>(ix, r));
    const uint32_t code = letter >= 0 ? (uint32_t)letter : 8u;
    if (code) atomicOr(&text4[p >> 3], code << (4 * (p & 7)));
  }
}

// the text as symbol indices, one byte per position (DevIndex::text8), by the same identity
template <int A>
__global__ __launch_bounds__(256) void text8_scatter_kernel(DevIndex ix, uint8_t* __restrict__ text8) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < ix.bwt_len; r += stride) {
    const uint64_t v = ix.dense_sa[r];
    text8[v ? v - 1 : ix.bwt_len - 1] = (uint8_t)symbol_at<A>(ix, r);
  }
}

// largest query q >= lo with hit_off[q] <= h (the query that owns hit h; queries without hits are skipped because their
// offset equals their successor's).  Needs hit_off[lo] <= h; hit_off has n + 1 entries and hit_off[n] = total > h.
// Gallops from lo: the owner of a tile's first hit is usually a few queries past the previous tile's.
__device__ __forceinline__ uint64_t owner_from(const uint64_t* __restrict__ hit_off, uint64_t lo, uint64_t n, uint64_t h) {
  uint64_t a = lo, step = 1;
  while (a + step < n && hit_off[a + step] <= h) { a += step; step <<= 1; }
  uint64_t hi = a + step < n ? a + step : n;
  while (hi - a > 1) { const uint64_t mid = (a + hi) >> 1; if (hit_off[mid] <= h) a = mid; else hi = mid; }
  return a;
}

// Hits in tiles of LOC_TILE; a block draws RUNS of consecutive tiles from an atomic head (run_len tiles at a time: the
// launcher picks it so that every block still gets several runs).  Only the first tile of a run searches the whole offset
// array for the query that owns its first hit (27 dependent loads at GRCh38 batch sizes -- per tile that chain was most
// of this kernel's time); the next tile's owner is read off the offsets the block already holds in LDS.  Per tile the
// offsets and range words of up to LOC_QCAP queries are staged in LDS and every hit finds its query there.  A hit whose
// row is a sampled one (or whose count pass left a text position) is emitted here; the others are flagged for the walk
// kernels, so every hit costs the same and the hits of a tile are dealt out statically.
template <int A>
__global__ __launch_bounds__(256) void locate_tile_kernel(DevIndex ix, const uint64_t* __restrict__ range_start, int rs_stride,
                                                          const uint64_t* __restrict__ hit_off, uint64_t n, uint64_t total,
                                                          const uint32_t* __restrict__ dense, uint32_t dense_ratio,
                                                          uint64_t* __restrict__ gpos, uint64_t* __restrict__ pos,
                                                          unsigned long long* __restrict__ tile_counter, uint32_t run_len) {
  __shared__ uint64_t s_off[LOC_QCAP + 1];
  __shared__ uint64_t s_sp[LOC_QCAP];
  __shared__ uint64_t s_starts[LOC_SEQ_LDS];
  __shared__ unsigned long long s_tile;
  __shared__ uint64_t s_q0;
  const bool seq_lds = pos && ix.nseq <= (uint64_t)LOC_SEQ_LDS;
  if (seq_lds)
    for (uint64_t t = threadIdx.x; t < ix.nseq; t += blockDim.x) s_starts[t] = ix.seq_starts[t];
  const uint64_t ntiles = (total + LOC_TILE - 1) / LOC_TILE;
  for (;;) {
    if (threadIdx.x == 0) {
      const unsigned long long t0 = atomicAdd(tile_counter, (unsigned long long)run_len);
      s_tile = t0;
      if (t0 < ntiles) {  // owner of the run's first hit: plain binary search over all queries
        const uint64_t h = t0 * LOC_TILE;
        uint64_t lo = 0, hi = n;
        while (hi - lo > 1) { const uint64_t mid = (lo + hi) >> 1; if (hit_off[mid] <= h) lo = mid; else hi = mid; }
        s_q0 = lo;
      }
    }
    __syncthreads();
    const uint64_t run0 = s_tile;
    if (run0 >= ntiles) break;
    const uint64_t run1 = run0 + run_len < ntiles ? run0 + run_len : ntiles;
    for (uint64_t tile = run0; tile < run1; tile++) {
      const uint64_t h0 = tile * LOC_TILE;
      const int tn = (int)(total - h0 < (uint64_t)LOC_TILE ? total - h0 : (uint64_t)LOC_TILE);
      const uint64_t h_last = h0 + (uint64_t)tn - 1;
      const uint64_t q0 = s_q0;
      const uint64_t nload = n - q0 < (uint64_t)LOC_QCAP ? n - q0 : (uint64_t)LOC_QCAP;  // queries q0 .. q0 + nload - 1
      for (uint64_t t = threadIdx.x; t <= nload; t += blockDim.x) s_off[t] = hit_off[q0 + t];
      __syncthreads();
      // do the staged queries own the whole tile?  (not when it spans more than LOC_QCAP queries, most of them without hits)
      const bool cached = s_off[nload] > h_last;
      uint64_t nq = nload;  // staged queries that own a hit of the tile: the range words of the others are not needed
      if (cached) {
        uint64_t lo = 0, hi = nload;
        while (hi - lo > 1) { const uint64_t mid = (lo + hi) >> 1; if (s_off[mid] <= h_last) lo = mid; else hi = mid; }
        nq = lo + 1;
        for (uint64_t t = threadIdx.x; t < nq; t += blockDim.x) s_sp[t] = range_start[(q0 + t) * rs_stride];
      }
      __syncthreads();
      for (int t = threadIdx.x; t < tn; t += blockDim.x) {
        const uint64_t h = h0 + (uint64_t)t;
        uint64_t rs, j;  // the owning query's range-start word and the index of this hit inside the query
        if (cached) {
          uint64_t lo = 0, hi = nq;
          while (hi - lo > 1) { const uint64_t mid = (lo + hi) >> 1; if (s_off[mid] <= h) lo = mid; else hi = mid; }
          rs = s_sp[lo];
          j = h - s_off[lo];
        } else {
          const uint64_t lo = owner_from(hit_off, q0, n, h);
          rs = range_start[lo * rs_stride];
          j = h - hit_off[lo];
        }
        const uint64_t rmode = rs >> RS_MODE_SHIFT;
        bool direct = rmode != RS_PLAIN;
        uint64_t row = 0, gd = 0;
        if (rmode == RS_SINGLE) {
          gd = rs & ((1ull << 40) - 1);  // the count pass already verified this match against the text
        } else if (rmode == RS_MULTI) {
          uint32_t mask = (uint32_t)(rs >> 48) & 0xffu;
          for (uint64_t t2 = 0; t2 < j; t2++) mask &= mask - 1;  // drop the j lowest set bits
          const uint32_t cand = (uint32_t)__ffs((int)mask) - 1u;
          gd = (uint64_t)ix.dense_sa[(uint32_t)rs + cand] - ((rs >> 32) & 0xffffull);
        } else if (rmode == RS_LCX) {
          // matched entries of the left-context index (up to 8 neighbours of lcx_rowpos: one line): hit j is the one with
          // the (j + 1)-th smallest BWT row -- ascending row order inside a query, src/fm_index.rs:521
          const uint32_t mask = (uint32_t)(rs >> 48) & 0xffu, base = (uint32_t)rs;
          uint64_t rp[8];
#pragma unroll
          for (int c = 0; c < 8; c++) rp[c] = (mask >> c) & 1u ? ix.lcx_rowpos[base + c] : ~0ull;
          uint64_t pick = 0;
#pragma unroll
          for (int c = 0; c < 8; c++) {
            uint32_t below = 0;
#pragma unroll
            for (int d = 0; d < 8; d++) below += (rp[d] >> 32) < (rp[c] >> 32) ? 1u : 0u;
            if (((mask >> c) & 1u) && below == (uint32_t)j) pick = rp[c];
          }
          gd = (pick & 0xffffffffull) - ((rs >> 32) & 0xffffull);
        } else {
          row = rs + j;
        }
        if (direct || row_is_sampled(ix, dense, dense_ratio, row)) {
          const uint64_t g = direct ? gd : walked_position(row_sample(ix, dense, dense_ratio, row), 0, ix.bwt_len);  // src/fm_index.rs:534, 0 steps
          gpos[h] = g;
          if (pos) {
            if (seq_lds) localise_lds(s_starts, ix.nseq, g, pos + 2 * h);
            else localise(ix, g, pos + 2 * h);
          }
        } else {
          gpos[h] = row | LOC_WALK_FLAG;  // a walk kernel finishes this hit,
          if (pos) pos[2 * h] = ~0ull;    // localise_walked_kernel its record / offset
        }
      }
      if (threadIdx.x == 0 && tile + 1 < run1) {  // owner of the next tile's first hit
        const uint64_t hn = h0 + (uint64_t)LOC_TILE;
        if (cached) {
          uint64_t lo = nq - 1, hi = nload + 1;   // s_off[nq - 1] <= h_last < hn
          while (hi - lo > 1) { const uint64_t mid = (lo + hi) >> 1; if (s_off[mid] <= hn) lo = mid; else hi = mid; }
          s_q0 = lo < nload ? q0 + lo : owner_from(hit_off, q0 + nload, n, hn);  // (lo == nload: the staged offsets end at or before hn)
        } else {
          s_q0 = owner_from(hit_off, q0, n, hn);
        }
      }
      __syncthreads();
    }
  }
}

// Second pass of locate: the hits whose row is not a sampled one walk the LF-mapping to the next sample
// (src/fm_index.rs:521-540).  Walk lengths are geometric (mean ratio - 1, tail ~6x that), so hits are not tied to
// blocks or tiles: every wave draws batches of LOC_WALK_BATCH consecutive hit indices from one device-wide counter and
// its lanes take the next index of the batch whenever their walk ends -- no lane idles behind a long walk except at the
// very end of the launch.  (Inside the tile kernel the same walks ran at ~40 % lane utilisation.)
constexpr int LOC_WALK_BATCH = 512;
template <int A>
__global__ __launch_bounds__(256) void locate_walk_kernel(DevIndex ix, uint64_t total, const uint32_t* __restrict__ dense, uint32_t dense_ratio,
                                                          uint64_t* __restrict__ gpos, uint64_t* __restrict__ pos,
                                                          unsigned long long* __restrict__ batch_counter) {
  const int lane = threadIdx.x & 63;
  const uint64_t lane_lt = (1ull << lane) - 1;
  uint64_t cur = 0, end = 0;  // wave-uniform: the unassigned rest of this wave's batch
  bool exhausted = false;     // wave-uniform: the counter has run past the last hit
  bool need = true;
  uint64_t h = 0, row = 0, steps = 0;
  for (;;) {
    const uint64_t nm = __ballot(need);
    if (nm) {
      if (cur == end && !exhausted) {
        unsigned long long base = 0;
        if (lane == 0) base = atomicAdd(batch_counter, (unsigned long long)LOC_WALK_BATCH);
        base = __shfl(base, 0, 64);
        cur = base < total ? base : total;
        end = base + LOC_WALK_BATCH < total ? base + LOC_WALK_BATCH : total;
        exhausted = cur == end;
      }
      if (exhausted && nm == ~0ull) break;  // nothing left to hand out and every lane is idle
      if (need) {
        const uint64_t idx = cur + (uint64_t)__popcll(nm & lane_lt);
        if (idx < end) {
          const uint64_t v = gpos[idx];
          if (v & LOC_WALK_FLAG) { h = idx; row = v & ~LOC_WALK_FLAG; steps = 0; need = false; }
        }
      }
      const uint64_t adv = cur + (uint64_t)__popcll(nm);
      cur = adv < end ? adv : end;
    }
    if (!need) {
      if (row_is_sampled(ix, dense, dense_ratio, row)) {
        gpos[h] = walked_position(row_sample(ix, dense, dense_ratio, row), steps, ix.bwt_len);  // src/fm_index.rs:534
        need = true;
      } else {
        row = backstep_scalar<A>(ix, row);
        steps++;
      }
    }
  }
}

// Third pass of locate, after a walk kernel: record / offset of the hits the tile pass deferred (pos[2h] == ~0).  Kept
// out of the walk kernels on purpose: the binary search over the record starts is a chain of dependent loads, and
// inside a state machine every wave iteration in which any quad emits would wait for all of it.
__global__ __launch_bounds__(256) void localise_walked_kernel(DevIndex ix, uint64_t total, const uint64_t* __restrict__ gpos,
                                                              uint64_t* __restrict__ pos) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t h = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; h < total; h += stride)
    if (pos[2 * h] == ~0ull) localise(ix, gpos[h], pos + 2 * h);
}

// SA values of the N block of the BWT (DevIndex::sa_nblock), by the chains of densify_sa_kernel: the thread of
// sampled row s walks LF until the next sampled row and records the rows of the window [lo, hi) it passes.
template <int A>
__global__ __launch_bounds__(256) void nblock_sa_kernel(DevIndex ix, uint64_t nsamples, uint32_t lo, uint32_t hi, uint32_t* __restrict__ out) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  const uint32_t fr = ix.sa_ratio;
  for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < nsamples; j += stride) {
    uint32_t row = (uint32_t)(j * fr);
    uint32_t v = (uint32_t)sa_sample(ix, j);
    for (;;) {
      if (row - lo < hi - lo) out[row - lo] = v;
      row = (uint32_t)backstep_scalar<A>(ix, row);
      if (row % fr == 0u) break;
      v--;
    }
  }
}

// Nucleotide walk kernel.  One hit per LANE, whole block per step: the lane fetches the 128-B block of its row with
// eight 16-B loads issued back to back (one line, one memory latency), then takes the BWT symbol and the rank from
// registers; the generic locate_walk_kernel above spends two dependent round trips per step (symbol, then rank) on
// ~14 separate 8-B loads.  Rows are u64, so it also serves indexes >= 2^32.
//
// Each lane is a three-state machine -- FETCH the next hit's row, WALK one backstep, EMIT at a sampled row -- and the
// lanes of a wave are in different states.  Written naively (load and use inside each branch) an iteration costs the
// SUM of the memory latencies of the branches present in the wave; here every iteration first issues the one load
// group each lane needs, under its state's predicate, and only then consumes the results.
//
// Measured on MI355X (GRCh38-scale, 5 M hits, ratio 8; locate = tile pass + walk + localise): walking inside the tile
// kernel 1.91 ms; this kernel 1.50 ms; a quad-cooperative variant (4 lanes per hit, 2 loads per lane, DPP reductions)
// 1.65 ms -- it was instruction-bound (~230 instructions per 16 steps), this one is bound by the texture path's
// per-lane line lookups (8 per step).
// LDS_SHARE: the blocks of a wave's 64 walks are fetched cooperatively -- eight lanes per block, so that one load
// instruction covers eight whole 128-B lines instead of 64 sixteen-byte pieces of 64 different lines (an eighth of the
// line lookups in the texture path) -- and handed to their lanes through a wave-private LDS tile.
// TALLY: tally[0] += LF steps taken, tally[1] += hits walked (the census the roofline figure of locate is computed from).
template <bool LDS_SHARE, bool TALLY = false>
__global__ __launch_bounds__(256) void locate_walk_nt_lane_kernel(DevIndex ix, uint64_t total, const uint32_t* __restrict__ dense,
                                                                  uint32_t dense_ratio, uint64_t* __restrict__ gpos,
                                                                  unsigned long long* __restrict__ batch_counter,
                                                                  unsigned long long* __restrict__ tally = nullptr) {
  constexpr int ROW = 9;  // 16-B pieces per tile row: 8 + 1 of padding against bank conflicts
  __shared__ ulonglong2 s_blk[LDS_SHARE ? 4 : 1][LDS_SHARE ? 64 * ROW : 1];
  const int lane = threadIdx.x & 63, wv_id = threadIdx.x >> 6;
  const uint64_t lane_lt = (1ull << lane) - 1;
  const uint64_t* __restrict__ blocks = ix.blocks;
  const uint64_t cA = ix.prefix_sums[1], cC = ix.prefix_sums[2], cG = ix.prefix_sums[3], cN = ix.prefix_sums[4], cT = ix.prefix_sums[5];
  const uint32_t* __restrict__ nblock = ix.sa_nblock;
  const uint64_t nspan = nblock ? cT - cN : 0ull;  // rows [cN, cN + nspan) resolve through nblock
  const uint64_t sa_bits = ix.sa_bits, bwt_len = ix.bwt_len, sentinel = ix.sentinel_row;
  const uint64_t ratio = dense ? (uint64_t)dense_ratio : (uint64_t)ix.sa_ratio;
  auto stops = [&](uint64_t row) { return ratio_divides(ratio, row) || row - cN < nspan; };
  uint64_t cur = 0, end = 0;  // wave-uniform: the unassigned rest of this wave's batch
  bool exhausted = false;     // wave-uniform
  enum { IDLE = 0, FETCH = 1, WALK = 2, EMIT = 3 };
  int state = IDLE;
  uint64_t h = 0, row = 0, steps = 0;
  unsigned long long t_steps = 0, t_hits = 0;
  for (;;) {
    const uint64_t nm = __ballot(state == IDLE);
    if (nm) {
      if (cur == end && !exhausted) {
        unsigned long long base = 0;
        if (lane == 0) base = atomicAdd(batch_counter, (unsigned long long)LOC_WALK_BATCH);
        base = __shfl(base, 0, 64);
        cur = base < total ? base : total;
        end = base + LOC_WALK_BATCH < total ? base + LOC_WALK_BATCH : total;
        exhausted = cur == end;
      }
      if (exhausted && nm == ~0ull) break;
      if (state == IDLE) {
        const uint64_t idx = cur + (uint64_t)__popcll(nm & lane_lt);
        if (idx < end) { h = idx; state = FETCH; }
      }
      const uint64_t adv = cur + (uint64_t)__popcll(nm);
      cur = adv < end ? adv : end;
    }
    // ---- issue
    uint64_t v = 0, s0 = 0, s1 = 0, ss = 0;
    ulonglong2 B[8];
#pragma unroll
    for (int j = 0; j < 8; j++) B[j] = ulonglong2{0, 0};
    if (state == FETCH) v = gpos[h];
    const uint64_t wm = LDS_SHARE ? __ballot(state == WALK) : 0ull;
    if (LDS_SHARE) {
      if (wm) {  // round r: the eight lanes 8j..8j+7 fetch the block of lane 8r + j, one 16-B piece each
        const unsigned long long myblk = state == WALK ? (unsigned long long)(row >> 8) : 0ull;
#pragma unroll
        for (int r = 0; r < 8; r++) {
          const int src = 8 * r + (lane >> 3);
          const unsigned long long b = __shfl(myblk, src, 64);
          if ((wm >> src) & 1ull) B[r] = reinterpret_cast<const ulonglong2*>(blocks + b * NT_BLOCK_WORDS)[lane & 7];
        }
      }
    } else if (state == WALK) {
      const ulonglong2* p = reinterpret_cast<const ulonglong2*>(blocks + (row >> 8) * NT_BLOCK_WORDS);
#pragma unroll
      for (int j = 0; j < 8; j++) B[j] = p[j];
    }
    if (state == EMIT) {
      if (row - cN < nspan) {
        s0 = nblock[row - cN];
      } else if (dense) {
        s0 = dense[ratio_quotient(ratio, row)];
      } else {  // src/compressed_suffix_array.rs:76-106
        const uint64_t off = ratio_quotient(ratio, row) * sa_bits;
        ss = off & 63;
        s0 = ix.sa_words[off >> 6];
        s1 = ix.sa_words[(off >> 6) + 1];  // the buffer has one word of slack
      }
    }
    asm volatile("" : "+v"(v), "+v"(s0), "+v"(s1), "+v"(B[0].x), "+v"(B[0].y), "+v"(B[1].x), "+v"(B[1].y), "+v"(B[2].x), "+v"(B[2].y),
                 "+v"(B[3].x), "+v"(B[3].y), "+v"(B[4].x), "+v"(B[4].y), "+v"(B[5].x), "+v"(B[5].y), "+v"(B[6].x), "+v"(B[6].y),
                 "+v"(B[7].x), "+v"(B[7].y));
    if (LDS_SHARE && wm) {  // pieces -> tile, then every walking lane picks up its own block
#pragma unroll
      for (int r = 0; r < 8; r++) s_blk[wv_id][(8 * r + (lane >> 3)) * ROW + (lane & 7)] = B[r];
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      if (state == WALK) {
#pragma unroll
        for (int j = 0; j < 8; j++) B[j] = s_blk[wv_id][lane * ROW + j];
      }
      __builtin_amdgcn_wave_barrier();
    }
    // ---- consume
    if (state == FETCH) {
      if (v & LOC_WALK_FLAG) { row = v & ~LOC_WALK_FLAG; steps = 0; state = stops(row) ? EMIT : WALK; }
      else state = IDLE;  // the tile pass already finished this hit
    } else if (state == EMIT) {
      uint64_t sample = s0;
      if (!(row - cN < nspan) && !dense) {
        sample = s0 >> ss;
        if (ss + sa_bits > 64) sample |= s1 << (64 - ss);
        if (sa_bits < 64) sample &= (1ull << sa_bits) - 1;
      }
      gpos[h] = walked_position(sample, steps, bwt_len);  // src/fm_index.rs:534
      if (TALLY) { t_steps += steps; t_hits++; }
      state = IDLE;
    } else if (state == WALK) {  // backstep, src/fm_index.rs:585-593; B[j] = {plane0[j], plane1[j]}, B[4 + j] = {plane2[j], milestone[j]}
      const uint64_t b = row >> 8;
      const int w = (int)((row >> 6) & 3), bit = (int)(row & 63);
      const uint64_t q0 = w == 0 ? B[0].x : (w == 1 ? B[1].x : (w == 2 ? B[2].x : B[3].x));
      const uint64_t q1 = w == 0 ? B[0].y : (w == 1 ? B[1].y : (w == 2 ? B[2].y : B[3].y));
      const uint64_t q2 = w == 0 ? B[4].x : (w == 1 ? B[5].x : (w == 2 ? B[6].x : B[7].x));
      const uint32_t code = (uint32_t)((q0 >> bit) & 1ull) | ((uint32_t)((q1 >> bit) & 1ull) << 1) | ((uint32_t)((q2 >> bit) & 1ull) << 2);
      steps++;
      if (code == 4u) {
        row = 0;  // '$': the walk continues from row 0
      } else {
        const int t = code == 6u ? 0 : (code == 5u ? 1 : (code == 3u ? 2 : (code == 1u ? 3 : -1)));  // A C G T, else N
        const uint32_t pc = t >= 0 ? code : 2u;  // as nt_index_of_code: anything else ranks as N (010)
        const uint64_t x0 = (pc & 1u) ? 0ull : ~0ull, x1 = (pc & 2u) ? 0ull : ~0ull, x2 = (pc & 4u) ? 0ull : ~0ull;
        const uint64_t last = ~0ull >> (63 - bit);
        uint32_t cnt = 0;
#pragma unroll
        for (int j = 0; j < 4; j++) {
          const uint64_t m = j < w ? ~0ull : (j == w ? last : 0ull);
          cnt += (uint32_t)__popcll((B[j].x ^ x0) & (B[j].y ^ x1) & (B[4 + j].x ^ x2) & m);
        }
        uint64_t ms, c0;
        if (t >= 0) {
          ms = t == 0 ? B[4].y : (t == 1 ? B[5].y : (t == 2 ? B[6].y : B[7].y));
          c0 = t == 0 ? cA : (t == 1 ? cC : (t == 2 ? cG : cT));
        } else {  // N: rows before the block that are neither A, C, G, T nor the single '$'
          ms = 256ull * b - (B[4].y + B[5].y + B[6].y + B[7].y) - (sentinel < 256ull * b ? 1ull : 0ull);
          c0 = cN;
        }
        row = c0 + ms + cnt - 1;
      }
      if (stops(row)) state = EMIT;
    }
  }
  if (TALLY && tally) {
    atomicAdd(&tally[0], t_steps);
    atomicAdd(&tally[1], t_hits);
  }
}

}  // namespace awry

#include "edit_kernels.hip.h"      // localise, backstep_scalar, symbol_at, ByteStream
#include "kernels_align.hip.h"     // edit_symbols, edit_owner, ByteStream
#include "kernels_chain.hip.h"     // localise, tally_add, Anchor
#include "kernels_chain_align.hip.h"  // Seed, Chain, ByteStream, edit_symbols, align_bam_op
#include "kernels_map.hip.h"       // Aln, Chain, Seed, localise
#include "kernels_split.hip.h"     // AlnClip, Chain, MapMode, map_key, localise
#include "kernels_pair.hip.h"      // MapRec, localise, EDIT_MAX_LEN
