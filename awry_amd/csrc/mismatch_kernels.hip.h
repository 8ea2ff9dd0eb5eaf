// mismatch_kernels.hip.h -- gfx950 kernels of substitution-tolerant and class-pattern count and locate (<= k mismatches, k <= 2).
//
// No counterpart in the reference (it answers exact queries only).  Semantics, as include/awry_hip.h states them: every query
// position stands for a set of symbol indices -- the one symbol of its byte (the map of alphabet.h: N, R, Y ... are the symbol
// N, X for amino) in the letter mode, the class of its letter (pattern_class of alphabet.h) in the class mode -- the distance
// of text position p is the number of j < L with text[p + j] outside the set of query[j], and p is an occurrence with <= k
// mismatches when its window holds no '$' and its distance is <= k.  A mismatching text symbol is any non-sentinel symbol
// outside the set (nucleotide A C G N T, amino the 21 symbols, X included).
//
// Search: backward search from the query's right end that branches over the symbols (a bounded DFS), one query per lane.
// Every loop iteration is ONE expansion -- the Occ of every symbol at the two rows (sp - 1, ep) of one node, from the same
// two block fetches one exact step costs (rank_all) -- after which the lane advances its own state machine:
//   * "expand": the node in hand (cur) is expanded; a child s of a node with mm mismatches is visited when s is in the set
//     of the node's next position or mm < k, and costs a mismatch when it is outside.  Children at depth L are leaves and
//     are counted (and, with EMIT, written) on the spot; otherwise the lane keeps the first child to visit as its next node
//     and, when other children remain, pushes the node with the set of those children (one frame);
//   * "derive": no node in hand -- the top frame's next child is derived from a re-rank of the frame's rows (the lines are
//     usually still in L2), and the frame is popped when that was its last child.
// VISITING ORDER: the children that cost a mismatch first, in ascending symbol index, then the children inside the set in
// ascending symbol index.  A node stays on the stack as a frame only while children of it remain to be visited.  A frame at a
// one-symbol position is therefore on the stack only while one of its mismatch children is being explored (at most k of
// them, MM_MAX_K), a frame at a class position while any but its last child is (at most one per class position), and nodes
// at depth L - 1 push nothing (their children are leaves): at most min(L - 1, class positions + k) frames.
// STACK: the two top frames live in named registers; no private array is indexed by the depth, so there is no scratch memory.
// Distinct matched strings of one length have disjoint row ranges, so the count of a query is the sum of its leaf widths per
// distance, and the locate pass sorts the leaves of a query by first row.  A lane that finishes takes the next query from a
// per-wave atomic cursor.
// CLASSES (the class mode; a mode compiles a class-only step in or not at all, nothing is decided at run time) adds:
//   * the table in LDS holds a pattern_class mask per byte value where the letter mode's holds the symbol index of
//     index_of_ascii (whose one bit is that mode's set), a byte that is no class letter is rejected (Q_NOT_CLASS_LETTER), and so is a pattern with more than PT_MAX_CLASS class positions (Q_CLASS_POSITIONS):
//     with that cap the stack holds at most PT_MAX_FRAMES = 18 frames;
//   * frames below the two in registers, which the letter mode's k <= 2 never needs, go to a workspace in HBM laid out
//     [level][field][grid lane], so the lanes of a wave that push the same level write adjacent words;
//   * a pattern whose search has taken max_exp expansions and needs another is abandoned: status Q_EXPANSION_CAP, counts 0;
//   * the census also keeps the deepest stack (tally[2]).
#pragma once
#include <type_traits>

#include "kernels.hip.h"

namespace awry {

constexpr int MM_MAX_K = 2;                                     // AWRY_MAX_MISMATCHES
constexpr int PT_MAX_CLASS = 16;                                // AWRY_MAX_CLASS_POSITIONS
constexpr int PT_MAX_FRAMES = PT_MAX_CLASS + MM_MAX_K;          // deepest stack
constexpr int PT_WS_LEVELS = PT_MAX_FRAMES - 2;                 // frames below the two in registers
constexpr int PT_WS_WORDS = 3 * PT_WS_LEVELS;                   // u64 words of workspace per grid lane
constexpr uint32_t PT_TAB_NON_ASCII = 0x80000000u, PT_TAB_SENTINEL = 0x40000000u;  // table words of bytes that are no letters

// Occ values of an alphabet: amino milestones are u32 (bwt_len < 2^32, layout.h), which halves the registers of 21 of them
template <int A> struct MmOcc { using type = uint64_t; };
template <> struct MmOcc<AMINO> { using type = uint32_t; };
template <int A> constexpr int mm_nsym() { return A == NUCLEOTIDE ? 5 : 21; }  // non-sentinel symbol indices 1 .. nsym

// Occ(s, row) inclusive of `row` for every non-sentinel symbol index s, into occ[s - 1]; one pass over the row's block (the
// planes are loaded once, each symbol is a plane predicate + popcount per 64-row slice).  row == ~0 (the row before row 0)
// gives all zeros.  Must equal rank_scalar<A>(ix, row, s) for every s (tests/test_mismatch_gpu.py).
template <int A>
__device__ __forceinline__ void rank_all(const DevIndex& ix, uint64_t row, typename MmOcc<A>::type* occ) {
  constexpr int NS = mm_nsym<A>(), NP = A == NUCLEOTIDE ? 3 : 5, BW = A == NUCLEOTIDE ? NT_BLOCK_WORDS : AA_BLOCK_WORDS;
  using O = typename MmOcc<A>::type;
  if (row == ~0ull) {
#pragma unroll
    for (int s = 0; s < NS; s++) occ[s] = 0;
    return;
  }
  const uint64_t b = row >> 8;
  const int p = (int)(row & 255);
  const uint64_t* blk = ix.blocks + b * BW;
  uint64_t pl[NP][4], m[4];
#pragma unroll
  for (int l = 0; l < 4; l++) {
    m[l] = slice_mask(p - 64 * l);
#pragma unroll
    for (int bb = 0; bb < NP; bb++) pl[bb][l] = blk[plane_word(A, bb, l)];
  }
#pragma unroll
  for (int s = 1; s <= NS; s++) {
    const uint32_t code = A == NUCLEOTIDE ? nt_code_of_index(s) : aa_code_of_index(s);
    uint32_t cnt = 0;
#pragma unroll
    for (int l = 0; l < 4; l++) {
      uint64_t pr = m[l];
#pragma unroll
      for (int bb = 0; bb < NP; bb++) pr &= ((code >> bb) & 1u) ? pl[bb][l] : ~pl[bb][l];
      cnt += (uint32_t)__popcll(pr);
    }
    occ[s - 1] = (O)milestone<A>(ix, blk, b, s) + (O)cnt;
  }
}

// device test hook: rank_all at rows[i] -> out[i * nsym + s - 1] (a row >= bwt_len gives zeros)
template <int A>
__global__ __launch_bounds__(256) void rank_all_kernel(DevIndex ix, const uint64_t* __restrict__ rows, uint64_t n, uint64_t* __restrict__ out) {
  constexpr int NS = mm_nsym<A>();
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    typename MmOcc<A>::type occ[NS];
    const uint64_t row = rows[i];
    rank_all<A>(ix, row < ix.bwt_len ? row : ~0ull, occ);  // rows past the end read nothing (zeros)
#pragma unroll
    for (int s = 0; s < NS; s++) out[i * NS + s] = occ[s];
  }
}

// leaf of the locate passes: key = first row of the range, value = (width << 2) | distance
__device__ __forceinline__ uint64_t mm_leaf_val(uint64_t width, uint32_t dist) { return (width << 2) | dist; }

// One DFS frame: a node (rows sp..ep, `depth` query symbols matched from the right, `mm` of them substituted) and the set of
// its children still to visit (bit s = symbol index s).
struct MmFrame {
  uint64_t sp, ep;
  uint32_t depth, mm, mask;
};

// Outputs (all nullable unless stated):
//   counts[q * (k + 1) + d]  occurrences of query q at exactly d mismatches (count passes)
//   totals[q]                sum over d (what the locate pass scans into hit offsets)
//   nleaves[q]               leaves of query q (what the locate pass scans into leaf offsets)
//   status[q]                Q_OK or why the query is rejected: Q_EMPTY, Q_NON_ASCII, Q_SENTINEL (as count_scalar_kernel), and
//                            with CLASSES Q_NOT_CLASS_LETTER, Q_CLASS_POSITIONS, Q_EXPANSION_CAP
//   EMIT: leaves of query q go to leaf_key / leaf_val [leaf_off[q], leaf_off[q + 1]) in DFS order; a slot at or beyond
//         leaf_off[q + 1] is never written (the bound is checked where the slot is reserved)
//   tally[0] += expansions (rank_all pairs), tally[1] += queries searched, with CLASSES tally[2] = max(tally[2], deepest
//   stack in frames) (untimed census); count passes only: the EMIT instantiations keep no census (its registers would cost
//   the nucleotide class one a wave per SIMD)
// max_exp, ws: CLASSES only (unread otherwise).  ws: PT_WS_WORDS * gridDim.x * blockDim.x u64 words, owned by this launch.
// cursor: u64 work-queue head, zero before the launch.
template <int A, bool CLASSES, bool EMIT>
__global__ __launch_bounds__(256) void count_dfs_kernel(DevIndex ix, const uint8_t* __restrict__ ascii, const uint64_t* __restrict__ off,
                                                        uint64_t n, int k, uint64_t max_exp, uint64_t* __restrict__ counts,
                                                        uint64_t* __restrict__ totals, uint64_t* __restrict__ nleaves,
                                                        uint8_t* __restrict__ status, const uint64_t* __restrict__ leaf_off,
                                                        uint64_t* __restrict__ leaf_key, uint64_t* __restrict__ leaf_val,
                                                        uint64_t* __restrict__ ws, unsigned long long* __restrict__ cursor,
                                                        unsigned long long* __restrict__ tally) {
  constexpr int NS = mm_nsym<A>();
  using O = typename MmOcc<A>::type;
  // the table of a query byte in LDS.  CLASSES: its class mask (bit s = symbol index s; PT_TAB_* for a byte that is no letter).
  // Letter mode: its symbol index in one byte (0 = a sentinel, 0xFF = no ASCII): 256 bytes, which the mode's speed at k = 0 needs
  // 
  using Word = std::conditional_t<CLASSES, uint32_t, uint8_t>;
  __shared__ Word tab[256];
  {
    const uint8_t a = (uint8_t)threadIdx.x;
    if (CLASSES) tab[a] = (Word)(a >= 128 ? PT_TAB_NON_ASCII : (a == '$' || a == '#') ? PT_TAB_SENTINEL : pattern_class(A, a));
    else tab[a] = (Word)(a >= 128 ? 0xFF : index_of_ascii(A, a));
  }
  __syncthreads();
  const uint32_t lane = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
  // CLASSES only (the letter mode has no workspace and reads neither): level l, field f of this lane is wsl[(3 l + f) * nlanes]
  const uint64_t nlanes = CLASSES ? (uint64_t)gridDim.x * blockDim.x : 0;
  uint64_t* const wsl = CLASSES ? ws + ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) : nullptr;

  bool busy = false, exhausted = false;
  uint64_t q = 0, qb = 0, L = 0, pexp = 0;
  uint64_t cnt0 = 0, cnt1 = 0, cnt2 = 0, nl = 0, wr = 0, wr_end = 0;
  bool have_cur = false;
  MmFrame cur{}, ft{}, fs{};
  int top = 0, deepest = 0;  // frames on the stack: ft is frame top - 1, fs frame top - 2, frame i < top - 2 is workspace level i
  unsigned long long n_exp = 0, n_q = 0;

  for (;;) {
    // ---- idle lanes take the next queries: one atomic per wave
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
          if (CLASSES) {
            uint32_t ncls = 0;
            for (uint64_t i = b; i < e; i++) {
              const uint32_t c = tab[ascii[i]];
              if (c == PT_TAB_NON_ASCII) st = Q_NON_ASCII;
              else if (c == PT_TAB_SENTINEL) { if (st != Q_NON_ASCII) st = Q_SENTINEL; }
              else if (c == 0) { if (st == Q_OK) st = Q_NOT_CLASS_LETTER; }
              else ncls += (c & (c - 1)) ? 1u : 0u;
            }
            if (st == Q_OK && ncls > (uint32_t)PT_MAX_CLASS) st = Q_CLASS_POSITIONS;
          } else {
            for (uint64_t i = b; i < e; i++) {
              const uint8_t s = tab[ascii[i]];
              if (s == 0xFF) st = Q_NON_ASCII;
              else if (s == 0 && st == Q_OK) st = Q_SENTINEL;
            }
          }
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
    if (!__ballot(busy)) continue;  // lanes that drew rejected queries draw again

    if (CLASSES && busy && pexp >= max_exp) {  // the search needs another expansion and has none left: abandoned
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
      // the query's set at this node's next position: the class mask, or the one bit of the letter's symbol index qw.  The
      // letter mode tests the index where it can: testing the set costs it 5 (nucleotide) and 21 (amino) VGPRs
      const uint32_t qw = tab[ascii[qb + (L - 1 - x.depth)]], cls = CLASSES ? qw : 1u << qw;
      const auto inside = [&](uint32_t s) -> uint32_t { return CLASSES ? (cls >> s) & 1u : (uint32_t)(s == qw); };
      const auto first_child = [&](uint32_t m) -> uint32_t {  // of the children m: the lowest outside the set, else the lowest inside
        const uint32_t mis = m & ~cls;
        return !CLASSES && !mis ? qw : (uint32_t)(__ffs((int)(mis ? mis : m)) - 1);
      };
      uint32_t c = 0;                                           // the child that becomes the node in hand
      bool take = false;
      if (have_cur) {
        const bool leaf = x.depth + 1 == L, can_mis = (int)x.mm < k;
        uint32_t mask = 0;
#pragma unroll
        for (int s = 1; s <= NS; s++) {
          const uint64_t w = (uint64_t)(hi[s - 1] - lo[s - 1]);
          const uint32_t in = inside((uint32_t)s);
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
          c = first_child(mask);
          const uint32_t rest = mask & ~(1u << c);
          if (rest) {  // push the node with its remaining children; top < the frame bound of the mode
            if (CLASSES && top >= 2 && top - 2 < PT_WS_LEVELS) {
              uint64_t* w = wsl + (uint64_t)(3 * (top - 2)) * nlanes;
              w[0] = fs.sp;
              w[nlanes] = fs.ep;
              w[2 * nlanes] = ((uint64_t)fs.depth << 32) | (fs.mm << 24) | fs.mask;
            }
            fs = ft;
            ft = MmFrame{x.sp, x.ep, x.depth, x.mm, rest};
            top++;
            if (CLASSES && !EMIT) deepest = top > deepest ? top : deepest;
          }
          take = true;
        }
      } else {
        c = first_child(x.mask);
        const uint32_t rest = x.mask & ~(1u << c);
        if (rest) {
          ft.mask = rest;
        } else {  // its last child: pop
          top--;
          ft = fs;
          if (CLASSES && top >= 2) {
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
        cur = MmFrame{cs + clo, cs + chi - 1, x.depth + 1, x.mm + (inside(c) ^ 1u), 0};
        have_cur = true;
      } else {
        have_cur = false;
      }
      if (!have_cur && top == 0) {  // query done
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
    if (CLASSES && deepest) atomicMax(&tally[2], (unsigned long long)deepest);
  }
}

// after the segmented sort: leaf widths (for the scan into per-leaf hit offsets)
__global__ __launch_bounds__(256) void mm_leaf_widths_kernel(const uint64_t* __restrict__ val, uint64_t n, uint64_t* __restrict__ width) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) width[i] = val[i] >> 2;
}

// every hit h takes the distance of the leaf that owns it (leaf_hit_off[j] <= h < leaf_hit_off[j + 1])
__global__ __launch_bounds__(256) void mm_hit_distance_kernel(const uint64_t* __restrict__ leaf_hit_off, const uint64_t* __restrict__ val,
                                                              uint64_t nleaf, uint64_t total, uint8_t* __restrict__ mm) {
  for (uint64_t h = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; h < total; h += (uint64_t)gridDim.x * blockDim.x) {
    uint64_t lo = 0, hi = nleaf;
    while (hi - lo > 1) { const uint64_t mid = (lo + hi) >> 1; if (leaf_hit_off[mid] <= h) lo = mid; else hi = mid; }
    mm[h] = (uint8_t)(val[lo] & 3u);
  }
}

}  // namespace awry
