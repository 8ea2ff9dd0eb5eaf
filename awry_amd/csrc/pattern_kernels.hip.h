// pattern_kernels.hip.h -- gfx950 kernels of class-pattern count and locate (IUPAC / residue classes, <= k mismatches, k <= 2).
//
// No counterpart in the reference.  Semantics, as include/awry_hip.h states them: a pattern is a string of class letters
// (pattern_class of alphabet.h: a set of symbol indices per letter), the distance of text position p is the number of j < L
// with text[p + j] outside the class of pattern[j], and p is an occurrence with <= k mismatches when its window holds no '$'
// and its distance is <= k.  A mismatching text symbol is any non-sentinel symbol outside the class.
//
// Search: count_mismatch_kernel's scaffold (mismatch_kernels.hip.h) -- one pattern per lane, a per-wave atomic cursor for
// refill, ONE expansion (rank_all pair) per loop iteration, leaves counted per distance and, with EMIT, written -- with the
// per-position test "symbol in class" instead of "symbol == letter":
//   * a child s of a node with mm mismatches is visited when (class >> s) & 1 || mm < k, and costs !((class >> s) & 1);
//   * VISITING ORDER: the children that cost a mismatch first, in ascending symbol index, then the children inside the class
//     in ascending symbol index.  A node stays on the stack as a frame only while children of it remain to be visited.  A
//     frame at a one-symbol position is therefore on the stack only while one of its mismatch children is being explored (at
//     most k of them), a frame at a class position while any but its last child is (at most one per class position), and
//     nodes at depth L - 1 push nothing (their children are leaves): at most min(L - 1, class positions + k) frames,
//     PT_MAX_FRAMES = 18 with the cap on class positions that lane refill enforces;
//   * the two top frames live in named registers (what the mismatch kernel's k <= 2 needs, so plain-letter patterns never
//     leave them); deeper frames go to a workspace in HBM laid out [level][field][grid lane], so the lanes of a wave that
//     push the same level write adjacent words.  No private array is indexed by the depth: no scratch memory;
//   * a pattern whose search has taken max_exp expansions and needs another is abandoned: status Q_EXPANSION_CAP, counts 0.
// Distinct matched strings have disjoint row ranges, so counts are sums of leaf widths and the locate pass sorts the leaves
// of a pattern by first row, exactly as for the mismatch kernel's leaves.
#pragma once
#include "mismatch_kernels.hip.h"

namespace awry {

constexpr int PT_MAX_CLASS = 16;                                // AWRY_MAX_CLASS_POSITIONS
constexpr int PT_MAX_FRAMES = PT_MAX_CLASS + MM_MAX_K;          // deepest stack
constexpr int PT_WS_LEVELS = PT_MAX_FRAMES - 2;                 // frames below the two in registers
constexpr int PT_WS_WORDS = 3 * PT_WS_LEVELS;                   // u64 words of workspace per grid lane
constexpr uint32_t PT_TAB_NON_ASCII = 0x80000000u, PT_TAB_SENTINEL = 0x40000000u;  // table words of bytes that are no letters

// Outputs as count_mismatch_kernel's, and:
//   status[q]   also Q_NOT_CLASS_LETTER, Q_CLASS_POSITIONS, Q_EXPANSION_CAP
//   tally[0] += expansions, tally[1] += patterns searched, tally[2] = max(tally[2], deepest stack in frames); count passes
//   only: the EMIT instantiations keep no census (its registers would cost the nucleotide one a wave per SIMD)
// ws: PT_WS_WORDS * gridDim.x * blockDim.x u64 words, owned by this launch.  cursor: u64 work-queue head, zero before the launch.
template <int A, bool EMIT>
__global__ __launch_bounds__(256) void count_pattern_kernel(DevIndex ix, const uint8_t* __restrict__ ascii, const uint64_t* __restrict__ off,
                                                            uint64_t n, int k, uint64_t max_exp, uint64_t* __restrict__ counts,
                                                            uint64_t* __restrict__ totals, uint64_t* __restrict__ nleaves,
                                                            uint8_t* __restrict__ status, const uint64_t* __restrict__ leaf_off,
                                                            uint64_t* __restrict__ leaf_key, uint64_t* __restrict__ leaf_val,
                                                            uint64_t* __restrict__ ws, unsigned long long* __restrict__ cursor,
                                                            unsigned long long* __restrict__ tally) {
  constexpr int NS = mm_nsym<A>();
  using O = typename MmOcc<A>::type;
  __shared__ uint32_t tab[256];
  {
    const uint8_t a = (uint8_t)threadIdx.x;
    tab[threadIdx.x] = a >= 128 ? PT_TAB_NON_ASCII : (a == '$' || a == '#') ? PT_TAB_SENTINEL : pattern_class(A, a);
  }
  __syncthreads();
  const uint32_t lane = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
  const uint64_t nlanes = (uint64_t)gridDim.x * blockDim.x;
  uint64_t* const wsl = ws + ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x);  // level l, field f: wsl[(3 l + f) * nlanes]

  bool busy = false, exhausted = false;
  uint64_t q = 0, qb = 0, L = 0, pexp = 0;
  uint64_t cnt0 = 0, cnt1 = 0, cnt2 = 0, nl = 0, wr = 0, wr_end = 0;
  bool have_cur = false;
  MmFrame cur{}, ft{}, fs{};
  int top = 0, deepest = 0;  // frames on the stack: ft is frame top - 1, fs frame top - 2, frame i < top - 2 is workspace level i
  unsigned long long n_exp = 0, n_q = 0;

  for (;;) {
    // ---- idle lanes take the next patterns: one atomic per wave
    const uint64_t want = __ballot(!busy && !exhausted);
    if (want) {
      const int leader = __ffsll((long long)want) - 1;
      unsigned long long base = 0;
      if ((int)lane == leader) base = atomicAdd(cursor, (unsigned long long)__popcll(want));
      base = ((unsigned long long)__builtin_amdgcn_readlane((int)(base >> 32), leader) << 32) |
             (unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)base, leader);
      if (!busy && !exhausted) {
        q = base + (uint64_t)__popcll(want & ((1ull << lane) - 1ull));
        if (q >= n) {
          exhausted = true;
        } else {
          const uint64_t b = off[q], e = off[q + 1];
          uint8_t st = e > b ? Q_OK : Q_EMPTY;
          uint32_t ncls = 0;
          for (uint64_t i = b; i < e; i++) {
            const uint32_t c = tab[ascii[i]];
            if (c == PT_TAB_NON_ASCII) st = Q_NON_ASCII;
            else if (c == PT_TAB_SENTINEL) { if (st != Q_NON_ASCII) st = Q_SENTINEL; }
            else if (c == 0) { if (st == Q_OK) st = Q_NOT_CLASS_LETTER; }
            else ncls += (c & (c - 1)) ? 1u : 0u;
          }
          if (st == Q_OK && ncls > (uint32_t)PT_MAX_CLASS) st = Q_CLASS_POSITIONS;
          if (status) status[q] = st;
          if (st != Q_OK) {
            if (counts) for (int d = 0; d <= k; d++) counts[q * (uint64_t)(k + 1) + d] = 0;
            if (totals) totals[q] = 0;
            if (nleaves) nleaves[q] = 0;
          } else {
            busy = true;
            qb = b;
            L = e - b;
            cnt0 = cnt1 = cnt2 = nl = pexp = 0;
            if (EMIT) { wr = leaf_off[q]; wr_end = leaf_off[q + 1]; }
            cur = MmFrame{0, ix.bwt_len - 1, 0, 0, 0};
            have_cur = true;
            top = 0;
            if (!EMIT) n_q++;
          }
        }
      }
    }
    if (!__ballot(busy) && !__ballot(!exhausted)) break;
    if (!__ballot(busy)) continue;  // lanes that drew rejected patterns draw again

    if (busy && pexp >= max_exp) {  // the search needs another expansion and has none left: abandoned
      if (status) status[q] = Q_EXPANSION_CAP;
      if (counts) for (int d = 0; d <= k; d++) counts[q * (uint64_t)(k + 1) + d] = 0;
      if (totals) totals[q] = 0;
      if (nleaves) nleaves[q] = 0;
      busy = false;
    } else if (busy) {
      // ---- the node whose rows this iteration ranks: the one in hand, or the top frame (derive its next child)
      const MmFrame x = have_cur ? cur : ft;
      O lo[NS], hi[NS];
      rank_all<A>(ix, x.sp - 1, lo);  // sp == 0 (the root) -> ~0 -> zeros
      rank_all<A>(ix, x.ep, hi);
      if (!EMIT) n_exp++;
      pexp++;
      const uint32_t cls = tab[ascii[qb + (L - 1 - x.depth)]];  // the pattern's class at this node's next position
      uint32_t c = 0;                                           // the child that becomes the node in hand
      bool take = false;
      if (have_cur) {
        const bool leaf = x.depth + 1 == L, can_mis = (int)x.mm < k;
        uint32_t mask = 0;
#pragma unroll
        for (int s = 1; s <= NS; s++) {
          const uint64_t w = (uint64_t)(hi[s - 1] - lo[s - 1]);
          const uint32_t in = (cls >> s) & 1u;
          if (w && (in || can_mis)) {
            if (leaf) {
              const uint32_t d = x.mm + (in ^ 1u);
              cnt0 += d == 0 ? w : 0;
              cnt1 += d == 1 ? w : 0;
              cnt2 += d == 2 ? w : 0;
              if (EMIT && wr < wr_end) {
                leaf_key[wr] = ix.prefix_sums[s] + (uint64_t)lo[s - 1];
                leaf_val[wr] = mm_leaf_val(w, d);
                wr++;
              }
              nl++;
            } else {
              mask |= 1u << s;
            }
          }
        }
        if (mask) {
          const uint32_t mis = mask & ~cls;
          c = (uint32_t)(__ffs((int)(mis ? mis : mask)) - 1);
          const uint32_t rest = mask & ~(1u << c);
          if (rest) {  // push the node with its remaining children; top < PT_MAX_FRAMES by the bound above
            if (top >= 2 && top - 2 < PT_WS_LEVELS) {
              uint64_t* w = wsl + (uint64_t)(3 * (top - 2)) * nlanes;
              w[0] = fs.sp;
              w[nlanes] = fs.ep;
              w[2 * nlanes] = ((uint64_t)fs.depth << 32) | (fs.mm << 24) | fs.mask;
            }
            fs = ft;
            ft = MmFrame{x.sp, x.ep, x.depth, x.mm, rest};
            top++;
            if (!EMIT) deepest = top > deepest ? top : deepest;
          }
          take = true;
        }
      } else {
        const uint32_t mis = x.mask & ~cls;
        c = (uint32_t)(__ffs((int)(mis ? mis : x.mask)) - 1);
        const uint32_t rest = x.mask & ~(1u << c);
        if (rest) {
          ft.mask = rest;
        } else {  // its last child: pop
          top--;
          ft = fs;
          if (top >= 2) {
            const uint64_t* w = wsl + (uint64_t)(3 * (top - 2)) * nlanes;
            const uint64_t meta = w[2 * nlanes];
            fs = MmFrame{w[0], w[nlanes], (uint32_t)(meta >> 32), (uint32_t)(meta >> 24) & 0xFFu, (uint32_t)meta & 0xFFFFFFu};
          }
        }
        take = true;
      }
      if (take) {
        uint64_t clo = 0, chi = 0;
#pragma unroll
        for (int s = 1; s <= NS; s++)
          if ((uint32_t)s == c) { clo = lo[s - 1]; chi = hi[s - 1]; }
        const uint64_t cs = ix.prefix_sums[c];
        cur = MmFrame{cs + clo, cs + chi - 1, x.depth + 1, x.mm + (((cls >> c) & 1u) ^ 1u), 0};
        have_cur = true;
      } else {
        have_cur = false;
      }
      if (!have_cur && top == 0) {  // pattern done
        if (counts) {
          uint64_t* cq = counts + q * (uint64_t)(k + 1);
          cq[0] = cnt0;
          if (k >= 1) cq[1] = cnt1;
          if (k >= 2) cq[2] = cnt2;
        }
        if (totals) totals[q] = cnt0 + cnt1 + cnt2;
        if (nleaves) nleaves[q] = nl;
        busy = false;
      }
    }
  }
  if (!EMIT && tally) {
    if (n_exp) atomicAdd(&tally[0], n_exp);
    if (n_q) atomicAdd(&tally[1], n_q);
    if (deepest) atomicMax(&tally[2], (unsigned long long)deepest);
  }
}

}  // namespace awry
