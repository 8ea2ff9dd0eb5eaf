// kernels_anchor.hip.h -- anchors: the greedy longest-match factorisation of a query, one ASCII query per lane.
// A part of kernels.hip.h (one header, cut by kernel family): included there, in order, and not on its own.
//
// No counterpart in the reference (it answers whole queries only).  The definition, as include/awry_hip.h states it: with
// occurs(b, e) = "q[b..e) has at least one occurrence",
//     e = L
//     while e > 0:
//         if not occurs(e-1, e): e -= 1; continue          # the letter itself is absent from the text
//         b = smallest b' such that occurs(b', e)          # backward search until the range would become empty
//         if e - b >= min_len: report (q_begin = b, q_len = e - b, start_row, count) = row range of q[b..e)
//         if b == 0: stop
//         e = b - skip
// Anchors come out right to left; shorter ones than min_len are not reported but still consume their letters.
#pragma once

namespace awry {

struct Anchor { uint32_t q_begin, q_len; uint64_t start_row, count; };  // == awry_anchor_t (checked in anchor_host.h)

// Status of the ASCII query bytes[qb .. qb + L): Q_EMPTY, Q_NON_ASCII (a byte >= 0x80), Q_SENTINEL ('$' / '#'), else Q_OK --
// the prologue of every kernel of this file and of kernels_smem.hip.h.  `ascii` is the lane's stream over `bytes`.
template <int A>
__device__ __forceinline__ uint8_t ascii_query_status(const uint8_t* __restrict__ bytes, ByteStream& ascii, const uint8_t* lut, uint64_t qb, uint32_t L) {
  uint8_t st = L ? Q_OK : Q_EMPTY;
  if (A == NUCLEOTIDE) {  // eight bytes at a time: any byte >= 0x80, any '$' or '#'
    constexpr uint64_t K7F = 0x7F7F7F7F7F7F7F7Full, K80 = 0x8080808080808080ull;
    uint64_t high = 0, sent = 0;
    for (uint32_t j = 0; j < L; j += 8) {
      uint64_t x;
      __builtin_memcpy(&x, bytes + qb + j, 8);
      if (L - j < 8) x &= (1ull << (8 * (L - j))) - 1;  // bytes past the query read as 0: neither test fires
      high |= x & K80;
      const uint64_t t1 = x ^ 0x2424242424242424ull, t2 = x ^ 0x2323232323232323ull;
      sent |= (((((t1 & K7F) + K7F) | t1) & K80) ^ K80) | (((((t2 & K7F) + K7F) | t2) & K80) ^ K80);
    }
    if (high) st = Q_NON_ASCII;
    else if (sent && st == Q_OK) st = Q_SENTINEL;
  } else {
    for (uint32_t j = 0; j < L; j++) {
      const uint8_t s = lut[ascii[qb + j]];
      if (s == 0xFF) st = Q_NON_ASCII;
      else if (s == 0 && st == Q_OK) st = Q_SENTINEL;
    }
  }
  return st;
}

// The table jump of a backward search that starts at e (needs e >= k = seed_k > 0): true, with [sp, ep] = the rows of
// q[e-k..e), when those k letters are all table digits and their entry states a row interval of count > 0 -- not when it is
// saturated, a position seed (.sp is a text position), an amino context entry, or empty.
template <int A>
__device__ __forceinline__ bool seed_rows_ending_at(const DevIndex& ix, ByteStream& ascii, const uint8_t* lut, uint64_t qb, uint32_t e, uint32_t k,
                                                    uint64_t& sp, uint64_t& ep) {
  uint64_t sidx = 0;
  bool digits = true;
  if (A == NUCLEOTIDE) {
    for (uint32_t j = 0; j < k; j++) {  // leftmost letter of the window least significant
      const int letter = nt_letter_of_index(lut[ascii[qb + e - k + j]]);
      digits = digits && letter >= 0;
      sidx |= (uint64_t)(letter & 3) << (2 * j);
    }
  } else {
    for (int j = (int)k - 1; j >= 0; j--) {
      const int letter = aa_letter_of_index(lut[ascii[qb + e - k + j]]);
      digits = digits && letter >= 0;
      sidx = sidx * AA_SEED_SIGMA + (uint64_t)(letter < 0 ? 0 : letter);
    }
  }
  if (!digits) return false;
  const SeedEntry se = seed_probe(ix.seed + sidx);
  const uint32_t cnt = A == NUCLEOTIDE ? seed_cnt(se) : aa_seed_cnt(se);
  const bool rows = cnt != 0 && cnt != (A == NUCLEOTIDE ? SEED_CNT_SAT : AA_SEED_CNT_SAT) && !(ix.seed_pos && cnt == 1) &&
                    !(A == NUCLEOTIDE ? seed_has_ctx(se) : aa_seed_is_ctx(se));
  if (!rows) return false;
  sp = se.sp;
  ep = (uint64_t)se.sp + cnt - 1;
  return true;
}

// Each lane runs a FLAT state machine over its query: one loop iteration either starts an anchor at e (the initial range
// from prefix_sums, or from one seed-table probe that states a row interval) or takes ONE step_scalar with the next letter
// to the left, into a second range, so that a step that empties the range is simply not committed.  There is no loop per
// anchor: the lanes of a wave restart at different letters, and a nested loop would make the wave wait for the longest
// anchor in hand at every restart.  State: e, i, the two ranges and the anchor counter -- no verify / LCX / text code here,
// the kernel is a chain of dependent 128-B lines per lane and what hides their latency is the number of resident chains.
//   FILL = 0: n_anchors[q] and status[q] (as count_scalar_kernel: != Q_OK marks a rejected query, which has 0 anchors)
//   FILL = 1: the identical walk; anchor j of query q goes to anchors[anchor_off[q] + j] (a slot at or beyond
//             anchor_off[q + 1] is never written); n_anchors / status are written where non-null
// Table jump (performance only): at an anchor start with e >= seed_k whose last seed_k letters are all table digits, the
// entry is used where it states a row interval of count > 0 -- not when it is saturated, a position seed (.sp is a text
// position), an amino context entry, or empty (the longest match is then shorter than seed_k and unknown): those start
// from the single letter.  Wide-row replicas (seed64) skip the table.
// tally (nullable census): [0] LF steps executed (failed ones included), [1] probes that supplied a range, [2] anchors reported.
// Registers: a step keeps the blocks of both rows (sp - 1, ep) in flight, 2 x 13 words nucleotide -- with the state above
// that is 96 VGPRs (5 waves per SIMD) nucleotide, ~120 (4 waves) amino, no scratch; the attribute below holds the
// nucleotide instantiations at 5 waves (the fill pass came out 2 registers over on its own).  DESIGN.md has the table.
template <int A, int FILL>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(A == NUCLEOTIDE ? 5 : 4, 8)))
void anchor_scalar_kernel(DevIndex ix, const uint8_t* __restrict__ ascii, const uint64_t* __restrict__ off, uint64_t n, uint32_t min_len,
                          uint32_t skip, uint64_t* __restrict__ n_anchors, const uint64_t* __restrict__ anchor_off,
                          Anchor* __restrict__ anchors, uint8_t* __restrict__ status, unsigned long long* __restrict__ tally) {
  __shared__ uint8_t lut[256];
  lut[threadIdx.x] = (uint8_t)(threadIdx.x >= 128 ? 0xFF : index_of_ascii(A, (uint8_t)threadIdx.x));
  __syncthreads();
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  const uint8_t* const ascii_bytes = ascii;
  const uint32_t k = ix.seed ? (uint32_t)ix.seed_k : 0u;
  for (uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; q < n; q += stride) {
    const uint64_t qb = off[q];
    const uint32_t L = (uint32_t)(off[q + 1] - qb);
    ByteStream ascii(ascii_bytes);  // shadows the pointer: same indexing, 8 bytes per load
    const uint8_t st = ascii_query_status<A>(ascii_bytes, ascii, lut, qb, L);
    uint32_t na = 0, t_steps = 0, t_probes = 0;
    if (st == Q_OK) {
      Anchor* const out = FILL ? anchors + anchor_off[q] : nullptr;                     // this query's slots,
      const uint32_t room = FILL ? (uint32_t)(anchor_off[q + 1] - anchor_off[q]) : 0u;  //   and how many it owns
      uint32_t e = L, i = L;   // the anchor in hand is q[i..e); i == e: none
      uint64_t sp = 1, ep = 0;
      for (;;) {
        bool ended = false;  // the anchor in hand cannot grow: its next letter empties the range, or it has reached letter 0
        if (i == e) {        // ---- start an anchor at e
          if (e == 0) break;
          const bool jumped = k && e >= k && seed_rows_ending_at<A>(ix, ascii, lut, qb, e, k, sp, ep);
          if (jumped) { i = e - k; t_probes++; }
          if (!jumped) {
            const int idx = lut[ascii[qb + e - 1]];
            sp = ix.prefix_sums[idx];
            ep = ix.prefix_sums[idx + 1] - 1;
            if (sp > ep) { e--; i = e; continue; }  // the letter itself is absent from the text
            i = e - 1;
          }
          ended = i == 0;
        } else {             // ---- one step with the next letter to the left
          uint64_t s2 = sp, e2 = ep;
          step_scalar<A>(ix, s2, e2, lut[ascii[qb + i - 1]]);
          t_steps++;
          if (s2 <= e2) { sp = s2; ep = e2; i--; ended = i == 0; }
          else ended = true;
        }
        if (ended) {
          if (e - i >= min_len) {
            if (FILL && na < room) out[na] = Anchor{i, e - i, sp, ep - sp + 1};
            na++;
          }
          if (i == 0) break;
          e = i - skip;  // skip = 0: the letter that failed ends the next anchor; 1: it is left out
          i = e;
        }
      }
    }
    if (n_anchors) n_anchors[q] = na;
    if (status) status[q] = st;
    if (tally) { tally_add(tally, 0, t_steps); tally_add(tally, 1, t_probes); tally_add(tally, 2, na); }
  }
}

// anchors -> what the locate pipeline takes: (start_row, end_row) pairs and the hits to locate per anchor (count, or 0
// for an anchor of more than max_hits rows, which keeps its record and gets no hits)
__global__ __launch_bounds__(256) void anchor_ranges_kernel(const Anchor* __restrict__ anchors, uint64_t n, uint64_t max_hits,
                                                            uint64_t* __restrict__ ranges, uint64_t* __restrict__ located) {
  for (uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; s < n; s += (uint64_t)gridDim.x * blockDim.x) {
    const Anchor a = anchors[s];
    ranges[2 * s] = a.start_row;
    ranges[2 * s + 1] = a.start_row + a.count - 1;
    located[s] = a.count <= max_hits ? a.count : 0;
  }
}

}  // namespace awry
