// kernels_quad.hip.h -- nucleotide quad primitives: a quad of lanes ranks one 128-B block; the start of a search from its seed entry; text windows for seed-and-verify.
// A part of kernels.hip.h (one header, cut by kernel family): included there, in order, and not on its own.
#pragma once

namespace awry {

// ------------------------------------------------------------------------------------------------
// quad-cooperative nucleotide path: packed 2-bit k-mers, seed table, persistent quads
// ------------------------------------------------------------------------------------------------

// sum over the 4 lanes of a quad; every lane receives the total.  32-bit rows: quad_perm DPP, no LDS
__device__ __forceinline__ uint32_t quad_sum(uint32_t v) {
  v += (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0xB1, 0xF, 0xF, true);  // quad_perm [1,0,3,2]
  v += (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x4E, 0xF, 0xF, true);  // quad_perm [2,3,0,1]
  return v;
}
// 64-bit rows (wide indexes)
__device__ __forceinline__ uint64_t quad_sum(uint64_t v) {
  v += __shfl_xor(v, 1, 64);
  v += __shfl_xor(v, 2, 64);
  return v;
}

// 2-bit letter (A0 C1 G2 T3) -> per-plane XOR masks of its 3-bit code (A110 C101 G011 T001)
struct NtXor { uint64_t x0, x1, x2; };
__device__ __forceinline__ NtXor nt_xor_of_letter(uint32_t c) {
  const uint32_t code = (0x1356u >> (4 * c)) & 7u;  // nibbles: A=6, C=5, G=3, T=1
  NtXor r;
  r.x0 = (code & 1u) ? 0ull : ~0ull;
  r.x1 = (code & 2u) ? 0ull : ~0ull;
  r.x2 = (code & 4u) ? 0ull : ~0ull;
  return r;
}

// letter j of a packed query (letter j in word j / 32, bits [2 (j % 32), + 2))
__device__ __forceinline__ uint32_t nt2_letter_at(const uint64_t* __restrict__ qw, int j) {
  return (uint32_t)(qw[j >> 5] >> (2 * (j & 31))) & 3u;
}

struct QuadBlock { ulonglong2 lo, hi; };  // lane l: lo = {plane0[l], plane1[l]}, hi = {plane2[l], milestone[l]}

// Row: the type of a BWT row -- uint32_t (bwt_len < 2^32) or uint64_t (wide rows); deduced from the caller's rows
template <class Row>
__device__ __forceinline__ QuadBlock quad_load(const uint64_t* __restrict__ blocks, Row b, int l) {
  const ulonglong2* p = reinterpret_cast<const ulonglong2*>(blocks + (uint64_t)b * NT_BLOCK_WORDS);
  QuadBlock q;
  q.lo = p[l];      // bytes [16 l, 16 l + 16) of the first half line
  q.hi = p[4 + l];  // bytes [64 + 16 l, ...) of the second half line
  return q;
}

// this lane's share of C-free rank(row, letter c): popcount of its slice + the milestone if it owns it
template <class Row>
__device__ __forceinline__ Row quad_rank_part(const QuadBlock& d, const NtXor& x, Row row, uint32_t c, int l) {
  const uint64_t pred = (d.lo.x ^ x.x0) & (d.lo.y ^ x.x1) & (d.hi.x ^ x.x2);
  const Row cnt = (Row)__popcll(pred & slice_mask((int)(row & 255u) - 64 * l));
  return cnt + ((uint32_t)l == c ? (Row)d.hi.y : (Row)0);
}

// one backward-search step for the quad's query: [sp, ep] -> [sp', ep'] with letter c (src/fm_index.rs:559-582)
template <class Row>
__device__ __forceinline__ void quad_step(const uint64_t* __restrict__ blocks, Row cl, Row& sp, Row& ep, uint32_t c, int l) {
  const Row r0 = sp - 1, r1 = ep;
  const Row b0 = r0 >> 8, b1 = r1 >> 8;
  QuadBlock d0 = quad_load(blocks, b0, l);
  QuadBlock d1 = d0;
  if (b1 != b0) d1 = quad_load(blocks, b1, l);  // most steps rank both rows in one block
  const NtXor x = nt_xor_of_letter(c);
  const Row v0 = quad_sum(quad_rank_part(d0, x, r0, c, l));
  const Row v1 = quad_sum(quad_rank_part(d1, x, r1, c, l));
  sp = cl + v0;
  ep = cl + v1 - 1;
}

// Where a search starts from its seed entry (32-bit rows): reads_body uses the first two, count_nt2_quad_kernel and
// count_nt2_quad4_kernel the third (the chunk, resume and wide kernels keep their own text).
// The range of an entry: its rows, or the empty range [1, 0] where it has none.  Returns the number of rows.
__device__ __forceinline__ uint32_t seed_entry_range(SeedEntry e, uint32_t& sp, uint32_t& ep) {
  const uint32_t scnt = seed_cnt(e);
  sp = scnt ? e.sp : 1u;
  ep = scnt ? e.sp + scnt - 1u : 0u;
  return scnt;
}
// A singleton entry keeps BWT[sp]: its row survives the next step only if that is the next letter, letter i - 1 of the query
// (at bit sh of w).  Entries of scnt != 1 rows and searches with no letter left (i == 0) are not touched.
__device__ __forceinline__ void seed_singleton_check(SeedEntry e, uint32_t scnt, uint64_t w, int sh, int i, uint32_t& sp, uint32_t& ep) {
  if (scnt == 1u && i > 0) {
    const uint32_t nc = (uint32_t)(w >> sh) & 3u;
    if (seed_sym(e) != (int)(nc == 3u ? 5u : nc + 1u)) { sp = 1u; ep = 0u; }
  }
}
// Start of a k-mer (one word w) with i0 letters left of its seed window: the checked range of its entry and i = i0; or
// i = -1 where the search has to start without the table -- a count the entry cannot represent, or a position seed
// (seed_pos: sp is a text position, not a row) that would have to be stepped.
__device__ __forceinline__ void kmer_seed_start(SeedEntry e, uint64_t w, int i0, uint32_t seed_pos, uint32_t& sp, uint32_t& ep, int& i) {
  const uint32_t scnt = seed_entry_range(e, sp, ep);
  i = i0;
  seed_singleton_check(e, scnt, w, 2 * (i - 1), i, sp, ep);
  if (scnt == SEED_CNT_SAT || (seed_pos && scnt == 1u && sp <= ep && i > 0)) i = -1;
}

// Seed-and-verify switch: compare the remaining i letters with the text instead of taking i more LF steps?
// A single candidate is verified at once (2 lines: SA + text, against one line per remaining letter); a range of
// 2..8 rows first takes `after` LF steps, which usually thin it out at one line each.
__device__ __forceinline__ bool verify_now(uint32_t cnt, int i, int steps_done, int after) {
  return cnt <= 8u && (int)(3u * cnt) <= i && (cnt == 1u || steps_done >= after);
}

// 16 packed 2-bit letters (low 32 bits of x) -> 16 nibbles holding the same letters
__device__ __forceinline__ uint64_t spread_letters16(uint64_t x) {
  x &= 0xFFFFFFFFull;
  x = (x | (x << 16)) & 0x0000FFFF0000FFFFull;
  x = (x | (x << 8)) & 0x00FF00FF00FF00FFull;
  x = (x | (x << 4)) & 0x0F0F0F0F0F0F0F0Full;
  x = (x | (x << 2)) & 0x3333333333333333ull;
  return x;
}

struct Text20 { uint32_t w[5]; };  // 5 consecutive u32 of the 4-bit text: any 32 symbols at any nibble offset

// A window of up to 32 text symbols, fetched now and compared later (so that several can be in flight per lane).
struct TextWin { Text20 t; int m, sh; };  // m symbols starting at nibble sh/4 of t
__device__ __forceinline__ TextWin text_window_load(const uint32_t* __restrict__ text4, uint64_t t0, int m) {
  TextWin w;
  w.m = m < 0 ? 0 : (m > 32 ? 32 : m);
  w.sh = 4 * (int)(t0 & 7);
  if (w.m > 0) w.t = *reinterpret_cast<const Text20*>(text4 + (t0 >> 3));
  else w.t = Text20{{0u, 0u, 0u, 0u, 0u}};
  return w;
}
// 1 = the window differs from the 32 letters of qword (its first m letters)
__device__ __forceinline__ uint32_t text_window_differs(const TextWin& w, uint64_t qword) {
  if (w.m == 0) return 0u;
  const Text20& t = w.t;
  const int sh = w.sh, m = w.m;
  const uint64_t a0 = (uint64_t)t.w[0] | ((uint64_t)t.w[1] << 32), a1 = (uint64_t)t.w[2] | ((uint64_t)t.w[3] << 32), a2 = t.w[4];
  const uint64_t lo = sh ? (a0 >> sh) | (a1 << (64 - sh)) : a0;
  const uint64_t hi = sh ? (a1 >> sh) | (a2 << (64 - sh)) : a1;
  const uint64_t qlo = spread_letters16(qword), qhi = spread_letters16(qword >> 32);
  const uint64_t mlo = m >= 16 ? ~0ull : ((1ull << (4 * m)) - 1);
  const uint64_t mhi = m <= 16 ? 0ull : (m >= 32 ? ~0ull : ((1ull << (4 * (m - 16))) - 1));
  return (((lo ^ qlo) & mlo) | ((hi ^ qhi) & mhi)) ? 1u : 0u;
}

// Does text[g + 32 j0' .. ) equal this lane's 32-letter query word?  Lane l of the quad compares window symbols
// [128 c + 32 l, +32) of a window of `len` symbols starting at text position g; returns 1 on a mismatch.
__device__ __forceinline__ uint32_t verify_part(const uint32_t* __restrict__ text4, uint64_t g, int len, int c, int l, uint64_t qword) {
  const int j0 = 128 * c + 32 * l;
  return text_window_differs(text_window_load(text4, g + (uint64_t)j0, len - j0), qword);
}

}  // namespace awry
