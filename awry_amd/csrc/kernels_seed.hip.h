// kernels_seed.hip.h -- seed tables: level 1, extend and finalize for the three table kinds; position seeds.
// A part of kernels.hip.h (one header, cut by kernel family): included there, in order, and not on its own.
#pragma once

namespace awry {

// Seed table, level by level: entry o of level j+1 (window letters w_0..w_j, index = sum w_t 4^t with the
// LAST query symbol most significant) is one step of its parent o >> 2 with letter o & 3.
// Entry: SeedEntry (32-bit rows) or SeedEntry64 (wide rows); the row type is that of the entry's fields.
template <class Entry>
__global__ __launch_bounds__(256) void seed_level1_kernel(DevIndex ix, Entry* __restrict__ out) {
  using Row = decltype(Entry::sp);
  if (blockIdx.x == 0 && threadIdx.x < 4) {
    const int idx = nt_index_of_letter((int)threadIdx.x);
    const uint64_t s = ix.prefix_sums[idx], e = ix.prefix_sums[idx + 1];
    out[threadIdx.x] = Entry{(Row)s, (Row)(e - s)};
  }
}

template <class Entry>
__global__ __launch_bounds__(256) void seed_extend_kernel(DevIndex ix, const Entry* __restrict__ parent,
                                                          Entry* __restrict__ child, uint64_t nchild) {
  using Row = decltype(Entry::sp);
  const int l = threadIdx.x & 3;
  const uint64_t nquads = ((uint64_t)gridDim.x * blockDim.x) >> 2;
  const Row cA = (Row)ix.prefix_sums[1], cC = (Row)ix.prefix_sums[2], cG = (Row)ix.prefix_sums[3], cT = (Row)ix.prefix_sums[5];
  for (uint64_t o = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 2; o < nchild; o += nquads) {
    const Entry p = parent[o >> 2];
    Entry r{p.sp, 0};
    if (p.cnt) {
      const uint32_t c = (uint32_t)(o & 3);
      const Row cl = c == 0 ? cA : (c == 1 ? cC : (c == 2 ? cG : cT));
      Row sp = p.sp, ep = p.sp + p.cnt - 1;
      quad_step(ix.blocks, cl, sp, ep, c, l);
      r.sp = sp;
      r.cnt = sp > ep ? (Row)0 : ep - sp + (Row)1;
    }
    if (l == 0) child[o] = r;
  }
}

// last pass over the finished table: pack the BWT symbol of singleton ranges and saturate oversized counts
// (intermediate levels keep plain 32-bit counts because a child is derived from its parent's exact range)
__global__ __launch_bounds__(256) void seed_finalize_kernel(DevIndex ix, SeedEntry* __restrict__ table, uint64_t nentries) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t o = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; o < nentries; o += stride) {
    SeedEntry e = table[o];
    if (e.cnt == 1u) e.cnt = 1u | ((uint32_t)symbol_at<NUCLEOTIDE>(ix, e.sp) << 29);
    else if (e.cnt >= SEED_CNT_SAT) e.cnt = SEED_CNT_SAT;
    else continue;
    table[o] = e;
  }
}

// wide rows: 61-bit counts never saturate; the BWT symbol of a singleton goes to bits 61..63 (SeedEntry64, layout.h)
__global__ __launch_bounds__(256) void seed64_finalize_kernel(DevIndex ix, SeedEntry64* __restrict__ table, uint64_t nentries) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t o = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; o < nentries; o += stride) {
    SeedEntry64 e = table[o];
    if (e.cnt != 1ull) continue;
    e.cnt = 1ull | ((uint64_t)symbol_at<NUCLEOTIDE>(ix, e.sp) << 61);
    table[o] = e;
  }
}

// Position seeds (DevIndex::seed_pos): every singleton entry's row is replaced by the text position of that row's
// suffix.  A query whose seed window occurs once in the text then needs no SA read: the entry itself says where the
// single candidate is, and the text decides (2 random lines per such query instead of 3).
// text4 != nullptr (nucleotide): where the SEED_CTX_LEN + extra letters in front of the occurrence exist and are all
// ACGT they go into the entry as well (SEED_CTX, layout.h).
// text8 != nullptr (amino): where the five residues in front of BWT[row]'s exist they go into the entry (AA_SEED_SPECIAL).
__global__ __launch_bounds__(256) void seed_rows_to_positions_kernel(SeedEntry* __restrict__ table, uint64_t nentries,
                                                                     const uint32_t* __restrict__ dense_sa, uint32_t cnt_mask,
                                                                     const uint32_t* __restrict__ text4, int extra,
                                                                     const uint8_t* __restrict__ text8 = nullptr) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  const int clen = SEED_CTX_LEN + extra;  // <= 30
  auto letters16 = [](uint64_t x) {  // 16 nibbles -> 16 2-bit letters
    x &= 0x3333333333333333ull;
    x = (x | (x >> 2)) & 0x0F0F0F0F0F0F0F0Full;
    x = (x | (x >> 4)) & 0x00FF00FF00FF00FFull;
    x = (x | (x >> 8)) & 0x0000FFFF0000FFFFull;
    return (x | (x >> 16)) & 0x00000000FFFFFFFFull;
  };
  for (uint64_t o = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; o < nentries; o += stride) {
    SeedEntry e = table[o];
    if (text8) {  // amino entry: plain singletons only (bit 26 clear, count 1)
      if ((e.cnt & (AA_SEED_SPECIAL | AA_SEED_CNT_SAT)) != 1u) continue;
      const uint32_t p = dense_sa[e.sp];
      e.sp = p;
      if (p >= (uint32_t)AA_SEED_CTX_LEN) {  // text8[p - 1] is the BWT symbol already held in bits 27..31
        uint32_t ctx = 0;
        for (int j = 0; j < AA_SEED_CTX_LEN - 1; j++) ctx |= (uint32_t)(text8[p - 2 - j] & 0x1Fu) << (5 * j);
        e.cnt = (e.cnt & 0xF8000000u) | AA_SEED_SPECIAL | ctx;
      }
      table[o] = e;
      continue;
    }
    if ((e.cnt & cnt_mask) != 1u) continue;  // cnt_mask: SEED_CNT_SAT (nt)
    const uint32_t p = dense_sa[e.sp];
    e.sp = p;
    if (text4 && p >= (uint32_t)clen) {
      const uint64_t t0 = (uint64_t)p - clen;  // clen nibbles from nibble t0: at most five words
      const Text20 t = *reinterpret_cast<const Text20*>(text4 + (t0 >> 3));
      const int sh = 4 * (int)(t0 & 7);
      const uint64_t a0 = (uint64_t)t.w[0] | ((uint64_t)t.w[1] << 32), a1 = (uint64_t)t.w[2] | ((uint64_t)t.w[3] << 32), a2w = t.w[4];
      const uint64_t lo = sh ? (a0 >> sh) | (a1 << (64 - sh)) : a0;   // nibbles 0..15
      uint64_t hi = sh ? (a1 >> sh) | (a2w << (64 - sh)) : a1;         // nibbles 16..31
      hi &= clen > 16 ? (~0ull >> (4 * (32 - clen))) : 0ull;          // only the first clen nibbles count
      const uint64_t lo_used = clen >= 16 ? lo : (lo & ((1ull << (4 * clen)) - 1));
      if (((lo_used | hi) & 0x8888888888888888ull) == 0) {  // all of them are A, C, G or T
        const uint64_t full = letters16(lo_used) | (letters16(hi) << 32);  // text[p - clen + j] in bits [2j, 2j + 2)
        const uint32_t far = extra ? (uint32_t)(full & ((1ull << (2 * extra)) - 1)) : 0u;
        e.sp = p | (extra ? far << (32 - 2 * extra) : 0u);
        e.cnt = (e.cnt & 0xE0000000u) | SEED_CTX | (uint32_t)((full >> (2 * extra)) & SEED_CNT_SAT);
      }
    }
    table[o] = e;
  }
}

// Amino seed table (the 21 searchable symbols: 20 standard residues and X; '$' is never part of a window).  Same construction as the
// nucleotide table with sigma = 21 (layout.h, AA_SEED_SIGMA): entry o of level j+1 = one step of parent o / 21 with letter o % 21 (the
// leftmost window letter is the least significant digit).  Final entries pack the count in bits 0..26 (saturating
// at AA_SEED_CNT_SAT) and, for singletons, the 5-bit symbol index of BWT[sp] in bits 27..31.
__global__ __launch_bounds__(256) void aa_seed_level1_kernel(DevIndex ix, SeedEntry* __restrict__ out) {
  if (blockIdx.x == 0 && threadIdx.x < AA_SEED_SIGMA) {
    const int idx = aa_index_of_letter((int)threadIdx.x);
    const uint64_t s = ix.prefix_sums[idx], e = ix.prefix_sums[idx + 1];
    out[threadIdx.x] = SeedEntry{(uint32_t)s, (uint32_t)(e - s)};
  }
}

__global__ __launch_bounds__(256) void aa_seed_extend_kernel(DevIndex ix, const SeedEntry* __restrict__ parent,
                                                             SeedEntry* __restrict__ child, uint64_t nchild) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t o = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; o < nchild; o += stride) {
    const SeedEntry p = parent[o / AA_SEED_SIGMA];
    SeedEntry r{p.sp, 0};
    if (p.cnt) {
      uint64_t sp = p.sp, ep = (uint64_t)p.sp + p.cnt - 1;
      step_scalar<AMINO>(ix, sp, ep, aa_index_of_letter((int)(o % AA_SEED_SIGMA)));
      r.sp = (uint32_t)sp;
      r.cnt = sp > ep ? 0u : (uint32_t)(ep - sp + 1);
    }
    child[o] = r;
  }
}

__global__ __launch_bounds__(256) void aa_seed_finalize_kernel(DevIndex ix, SeedEntry* __restrict__ table, uint64_t nentries) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t o = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; o < nentries; o += stride) {
    SeedEntry e = table[o];
    if (e.cnt == 1u) e.cnt = 1u | ((uint32_t)symbol_at<AMINO>(ix, e.sp) << 27);
    else if (e.cnt >= 2u && e.cnt <= 4u) {  // the set of BWT symbols over the entry's rows (AA_SEED_MULTI, layout.h)
      uint32_t mask = 0;
      for (uint32_t j = 0; j < e.cnt; j++) mask |= 1u << symbol_at<AMINO>(ix, (uint64_t)e.sp + j);
      e.cnt = AA_SEED_SPECIAL | AA_SEED_MULTI | ((e.cnt - 2u) << 22) | mask;
    }
    else if (e.cnt >= AA_SEED_CNT_SAT) e.cnt = AA_SEED_CNT_SAT;
    else continue;
    table[o] = e;
  }
}

}  // namespace awry
