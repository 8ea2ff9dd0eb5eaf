// kernels_smem.hip.h -- SMEMs: all super-maximal exact matches of a query, one ASCII query per lane.
// A part of kernels.hip.h (one header, cut by kernel family): included there, in order, and not on its own.
//
// No counterpart in the reference (it answers whole queries only).  The definition, as include/awry_hip.h states it: with
// occurs(b, e) = "q[b..e) has at least one occurrence", an SMEM of a query of L letters is a pair (b, e), 0 <= b < e <= L, with
//     occurs(b, e)  and  (b == 0 or not occurs(b-1, e))  and  (e == L or not occurs(b, e+1))
// -- a match contained in no other match of the query.  Found right to left without a bidirectional index:
//     x = L - 1; top = L                                   # x: the letter the next SMEM must cover
//     while x >= 0:
//         if q[x] is absent from the text: x -= 1; continue
//         e = largest e' <= top with occurs(x, e')         # forward extension
//         b = smallest b' with occurs(b', e)               # backward search from e, as the anchor kernel does
//         report (b, e) if e - b >= min_len
//         x = b - 1; top = e - 1
// (b, e) is right-maximal: e < top means q[x..e+1) does not occur and b <= x; e == top < L means the SMEM before it,
// (b', top + 1) with b' = x + 1 > b, would otherwise have started at b.
#pragma once

namespace awry {

enum { SMEM_FWD_SA = 0, SMEM_FWD_LF = 1 };

// Common prefix of the suffix text8[p ..] with q[x .. x + cap), from letter m on (the first m are known to be equal; m < cap).
// -> its length (<= cap); less = the suffix sorts before the query (set where the length is < cap).  The comparison ends at
// or before the text's '$' (index 0), which no query holds; text8 and the query bytes are readable 8 bytes past their end.
template <int A>
__device__ __forceinline__ uint32_t suffix_lcp(const uint8_t* __restrict__ text8, uint64_t p, const uint8_t* __restrict__ q, ByteStream& ascii,
                                               uint64_t qx, uint32_t m, uint32_t cap, const uint8_t* lut, bool& less) {
  if (A == NUCLEOTIDE) {
    for (;;) {
      uint64_t tw, qw;
      __builtin_memcpy(&tw, text8 + p + m, 8);
      __builtin_memcpy(&qw, q + qx + m, 8);
      const uint64_t qi = nt_indices8(qw), d = tw ^ qi;
      const uint32_t rem = cap - m;
      if (d) {
        const uint32_t f = (uint32_t)__builtin_ctzll(d) >> 3;  // the first byte that differs
        if (f < rem) {
          less = (uint8_t)(tw >> (8 * f)) < (uint8_t)(qi >> (8 * f));
          return m + f;
        }
      }
      if (rem <= 8) return cap;
      m += 8;
    }
  }
  ByteStream t(text8);
  for (; m < cap; m++) {
    const uint8_t a = t[p + m], b = lut[ascii[qx + m]];
    if (a != b) { less = a < b; return m; }
  }
  return cap;
}

// Each lane runs a FLAT state machine over its query, as anchor_scalar_kernel does and for the same reason: one loop
// iteration is one suffix comparison, one step_scalar, or one cheap transition, and there is no loop per SMEM.  Phases:
//   NEXT  the letter x = xe - 1 the next SMEM must cover: absent from the text -> pass over it (and top with it); else one
//         forward extension
//   FWD   e = the largest e' <= top such that q[x..e') occurs, in one of two forms with the same result:
//         SMEM_FWD_SA  (dense_sa at ratio 1 and text8 resident) binary search for q[x..top) among the rows of the bucket of
//                      q[x]; every iteration compares ONE suffix text8 + dense_sa[mid] with the query.  llo / lhi are the
//                      common-prefix lengths at the two bounds: the comparison starts at their minimum, and e - x is their
//                      maximum when the bounds meet (the neighbours of the insertion point have both been compared, and
//                      the longest common prefix over a sorted bucket is at one of them); a suffix that holds all of
//                      q[x..top) ends the search at once.
//         SMEM_FWD_LF  (any replica) the predicate occurs(x, e') is monotone in e': probe e' = top first, then bisect
//                      [flo, fhi]; a probe is a plain backward search from e' down to x, one step_scalar per iteration.  When
//                      the probe that decides e succeeds, its range is the row interval of q[x..e) and BACK continues from it.
//   BACK  b = the smallest b' such that q[b'..e) occurs: the anchor kernel's walk from e (table jump included) into a
//         second range, so that the step that empties the range is not committed; then the record, x = b - 1, top = e - 1.
//   FILL = 0: n_smems[q] and status[q];  FILL = 1: the identical walk, record j of query q goes to smems[smem_off[q] + j] (a slot
//   at or beyond smem_off[q + 1] is never written) -- the buffer contract and status codes of anchor_scalar_kernel.
// tally (nullable census): [0] LF steps executed (failed ones included), [1] suffixes compared by the SA search, [2] forward
// extensions performed, [3] SMEMs reported.  The SA form takes LF steps in BACK only; with seed_k == 0 every extension
// costs e - b - 1 steps that commit and, unless b == 0, the one that fails:
//     tally[0] == sum over all extensions of (e - b - 1) + #(extensions with b > 0)
// and at min_len == 1 the extensions are exactly the reported records.
// Registers: a lane keeps what the anchor kernel keeps (two ranges, the blocks of two rows in flight during a step) plus
// x, top and four words of search state.  The kernel is a chain of dependent loads per lane -- dense_sa[mid], then the text
// line it names; or the two block lines of a step -- with nothing to overlap inside a lane, so what hides the latency is
// the number of resident waves.  On their own the instantiations need 112..116 VGPRs nucleotide and 141..145 amino, one
// occupancy step below the anchor kernel (96 / ~123).  Held at the anchor kernel's 5 / 4 waves per SIMD they spill 10..37
// registers (44..76 B of scratch per lane) inside the state machine, where every spill is one more memory round trip in the
// chain that bounds the kernel; waves_per_eu therefore asks for 4 waves nucleotide (<= 128 VGPRs) and 3 amino (<= 170), at
// which nothing spills (DESIGN.md has the table).
template <int A, int FWD, int FILL>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(A == NUCLEOTIDE ? 4 : 3, 8)))
void smem_scalar_kernel(DevIndex ix, const uint8_t* __restrict__ ascii, const uint64_t* __restrict__ off, uint64_t n, uint32_t min_len,
                        uint64_t* __restrict__ n_smems, const uint64_t* __restrict__ smem_off, Anchor* __restrict__ smems,
                        uint8_t* __restrict__ status, unsigned long long* __restrict__ tally) {
  __shared__ uint8_t lut[256];
  lut[threadIdx.x] = (uint8_t)(threadIdx.x >= 128 ? 0xFF : index_of_ascii(A, (uint8_t)threadIdx.x));
  __syncthreads();
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  const uint8_t* const ascii_bytes = ascii;
  const uint32_t k = ix.seed ? (uint32_t)ix.seed_k : 0u;
  enum { NEXT = 0, FWD_RUN = 1, BACK = 2 };
  for (uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; q < n; q += stride) {
    const uint64_t qb = off[q];
    const uint32_t L = (uint32_t)(off[q + 1] - qb);
    ByteStream ascii(ascii_bytes);  // shadows the pointer: same indexing, 8 bytes per load
    const uint8_t st = ascii_query_status<A>(ascii_bytes, ascii, lut, qb, L);
    uint32_t ns = 0, t_steps = 0, t_sa = 0, t_fwd = 0;
    if (st == Q_OK) {
      Anchor* const out = FILL ? smems + smem_off[q] : nullptr;                     // this query's slots,
      const uint32_t room = FILL ? (uint32_t)(smem_off[q + 1] - smem_off[q]) : 0u;  //   and how many it owns
      uint32_t xe = L, top = L;  // x + 1, and the largest end the next SMEM may have
      uint32_t e = L, i = L;     // BACK: the match in hand is q[i..e); i == e: none yet
      uint64_t sp = 1, ep = 0;
      uint32_t lo = 0, hi = 0, llo = 0, lhi = 0;  // SA form: the insertion point is in rows [lo, hi]; common prefixes at the bounds
      uint32_t flo = 0, fhi = 0, fe = 0, fi = 0;  // LF form: occurs(x, flo), e <= fhi; the probe in hand is q[fi..fe), fi == fe: none yet
      int phase = NEXT;
      for (;;) {
        if (phase == NEXT) {
          if (xe == 0) break;
          const int idx = lut[ascii[qb + xe - 1]];
          const uint64_t c0 = ix.prefix_sums[idx], c1 = ix.prefix_sums[idx + 1];
          if (c0 >= c1) {  // the letter itself is absent from the text: no SMEM reaches across it
            xe--;
            top = xe;
            continue;
          }
          t_fwd++;
          if (top == xe) {  // nothing to extend into
            e = top; i = e; phase = BACK;
          } else if (FWD == SMEM_FWD_SA) {
            lo = (uint32_t)c0; hi = (uint32_t)c1; llo = 1; lhi = 1;  // every suffix of the bucket shares q[x]
            phase = FWD_RUN;
          } else {
            flo = xe; fhi = top; fe = top; fi = fe;
            phase = FWD_RUN;
          }
        } else if (phase == FWD_RUN && FWD == SMEM_FWD_SA) {  // ---- one suffix against q[x..top)
          const uint32_t x = xe - 1, cap = top - x, mid = lo + ((hi - lo) >> 1);
          bool less = false;
          const uint32_t m = suffix_lcp<A>(ix.text8, ix.dense_sa[mid], ascii_bytes, ascii, qb + x, llo < lhi ? llo : lhi, cap, lut, less);
          t_sa++;
          if (m == cap) { llo = cap; lo = hi; }
          else if (less) { lo = mid + 1; llo = m; }
          else { hi = mid; lhi = m; }
          if (lo == hi) { e = x + (llo > lhi ? llo : lhi); i = e; phase = BACK; }
        } else if (phase == FWD_RUN) {                        // ---- one step of the probe q[x..fe)
          const uint32_t x = xe - 1;
          bool ok = false, failed = false;
          if (fi == fe) {
            const int idx = lut[ascii[qb + fe - 1]];
            sp = ix.prefix_sums[idx];
            ep = ix.prefix_sums[idx + 1] - 1;
            if (sp > ep) failed = true;
            else { fi = fe - 1; ok = fi == x; }
          } else {
            uint64_t s2 = sp, e2 = ep;
            step_scalar<A>(ix, s2, e2, lut[ascii[qb + fi - 1]]);
            t_steps++;
            if (s2 <= e2) { sp = s2; ep = e2; fi--; ok = fi == x; }
            else failed = true;
          }
          if (ok) flo = fe;
          if (failed) fhi = fe - 1;
          if (ok || failed) {
            if (flo == fhi) {  // decided; after a probe that succeeded [sp, ep] is the row interval of q[x..e)
              e = flo; i = ok ? x : e; phase = BACK;
            } else {
              fe = flo + ((fhi - flo + 1) >> 1);
              fi = fe;
            }
          }
        } else {                                              // ---- BACK, the anchor kernel's walk
          bool ended = false;  // the match in hand cannot grow: its next letter empties the range, or it has reached letter 0
          if (i == e) {
            const bool jumped = k && e >= k && seed_rows_ending_at<A>(ix, ascii, lut, qb, e, k, sp, ep);
            if (jumped) {
              i = e - k;
            } else {
              const int idx = lut[ascii[qb + e - 1]];
              sp = ix.prefix_sums[idx];
              ep = ix.prefix_sums[idx + 1] - 1;
              i = e - 1;
            }
            ended = i == 0;
          } else if (i == 0) {
            ended = true;  // the LF form's probe already reached letter 0
          } else {
            uint64_t s2 = sp, e2 = ep;
            step_scalar<A>(ix, s2, e2, lut[ascii[qb + i - 1]]);
            t_steps++;
            if (s2 <= e2) { sp = s2; ep = e2; i--; ended = i == 0; }
            else ended = true;
          }
          if (ended) {
            if (e - i >= min_len) {
              if (FILL && ns < room) out[ns] = Anchor{i, e - i, sp, ep - sp + 1};
              ns++;
            }
            if (i == 0) break;
            xe = i;
            top = e - 1;
            phase = NEXT;
          }
        }
      }
    }
    if (n_smems) n_smems[q] = ns;
    if (status) status[q] = st;
    if (tally) { tally_add(tally, 0, t_steps); tally_add(tally, 1, t_sa); tally_add(tally, 2, t_fwd); tally_add(tally, 3, ns); }
  }
}

}  // namespace awry
