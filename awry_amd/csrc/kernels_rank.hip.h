// kernels_rank.hip.h -- rank and text primitives: seed probe, scalar rank / step / backstep, SA samples, query bytes against the text.
// A part of kernels.hip.h (one header, cut by kernel family): included there, in order, and not on its own.
#pragma once

namespace awry {

// A seed-table probe reads 8 bytes of a line nobody will touch again (the table is 10..140 GB and the probes are random):
// loaded non-temporally, so that the line does not displace the streams that do have locality (query words, counts,
// survivor lists) from L2 / Infinity Cache.  Measured on the headline batch: 33.5 -> 35.9 G queries/s.
__device__ __forceinline__ SeedEntry seed_probe(const SeedEntry* __restrict__ p) {
  const unsigned long long raw = __builtin_nontemporal_load(reinterpret_cast<const unsigned long long*>(p));
  return SeedEntry{(uint32_t)raw, (uint32_t)(raw >> 32)};
}

// ------------------------------------------------------------------------------------------------
// scalar helpers (one lane does a whole rank)
// ------------------------------------------------------------------------------------------------

// inclusive mask of bits 0..=t of a 64-symbol slice; t < 0 -> none, t >= 63 -> all
__device__ __forceinline__ uint64_t slice_mask(int t) {
  uint64_t m = ~0ull >> (63 - (t > 63 ? 63 : (t < 0 ? 0 : t)));
  return t < 0 ? 0ull : m;
}

template <int A>
__device__ __forceinline__ uint64_t slice_pred(const uint64_t* blk, int l, uint32_t code) {
  uint64_t pr = ~0ull;
#pragma unroll
  for (int b = 0; b < (A == NUCLEOTIDE ? 3 : 5); b++) {
    uint64_t x = ((code >> b) & 1u) ? 0ull : ~0ull;
    pr &= blk[plane_word(A, b, l)] ^ x;
  }
  return pr;
}

// milestone of symbol index `idx` at the start of block `b` (exclusive prefix count, src/fm_index.rs:212-217)
template <int A>
__device__ __forceinline__ uint64_t milestone(const DevIndex& ix, const uint64_t* blk, uint64_t b, int idx) {
  if (A == NUCLEOTIDE) {
    int letter = nt_letter_of_index(idx);
    if (letter >= 0) return blk[nt_ms_word(letter)];
    // N is derived: rows before the block that are neither A,C,G,T nor the single '$'
    uint64_t sum = blk[nt_ms_word(0)] + blk[nt_ms_word(1)] + blk[nt_ms_word(2)] + blk[nt_ms_word(3)];
    return 256ull * b - sum - (ix.sentinel_row < 256ull * b ? 1ull : 0ull);
  }
  int t = idx - 1;
  return (blk[aa_ms_word(t)] >> (32 * aa_ms_half(t))) & 0xffffffffull;
}

// Occ(idx, row) inclusive of `row`: src/bwt.rs:338-357
template <int A>
__device__ __forceinline__ uint64_t rank_scalar(const DevIndex& ix, uint64_t row, int idx) {
  const uint64_t b = row >> 8;
  const int p = (int)(row & 255);
  const uint64_t* blk = ix.blocks + b * (A == NUCLEOTIDE ? NT_BLOCK_WORDS : AA_BLOCK_WORDS);
  const uint32_t code = A == NUCLEOTIDE ? nt_code_of_index(idx) : aa_code_of_index(idx);
  uint32_t cnt = 0;
#pragma unroll
  for (int l = 0; l < 4; l++) cnt += (uint32_t)__popcll(slice_pred<A>(blk, l, code) & slice_mask(p - 64 * l));
  return milestone<A>(ix, blk, b, idx) + cnt;
}

// symbol index stored at BWT row `row`: src/bwt.rs:307-325
template <int A>
__device__ __forceinline__ int symbol_at(const DevIndex& ix, uint64_t row) {
  const uint64_t* blk = ix.blocks + (row >> 8) * (A == NUCLEOTIDE ? NT_BLOCK_WORDS : AA_BLOCK_WORDS);
  const int l = (int)((row >> 6) & 3), bit = (int)(row & 63);
  uint32_t code = 0;
#pragma unroll
  for (int b = 0; b < (A == NUCLEOTIDE ? 3 : 5); b++) code |= (uint32_t)((blk[plane_word(A, b, l)] >> bit) & 1ull) << b;
  return A == NUCLEOTIDE ? nt_index_of_code(code) : aa_index_of_code(code);
}

// src/fm_index.rs:559-582
template <int A>
__device__ __forceinline__ void step_scalar(const DevIndex& ix, uint64_t& sp, uint64_t& ep, int idx) {
  const uint64_t c = ix.prefix_sums[idx];
  const uint64_t s2 = c + rank_scalar<A>(ix, sp - 1, idx);
  ep = c + rank_scalar<A>(ix, ep, idx) - 1;
  sp = s2;
}

// src/fm_index.rs:585-593
template <int A>
__device__ __forceinline__ uint64_t backstep_scalar(const DevIndex& ix, uint64_t row) {
  int idx = symbol_at<A>(ix, row);
  if (idx == 0) return 0;
  return ix.prefix_sums[idx] + rank_scalar<A>(ix, row, idx) - 1;
}

// src/compressed_suffix_array.rs:76-106
__device__ __forceinline__ uint64_t sa_sample(const DevIndex& ix, uint64_t sample) {
  const uint64_t bits = ix.sa_bits;
  if (bits == 0) return 0;
  const uint64_t off = sample * bits, w = off >> 6, s = off & 63;
  uint64_t v = ix.sa_words[w] >> s;
  if (s + bits > 64) v |= ix.sa_words[w + 1] << (64 - s);
  return bits >= 64 ? v : (v & ((1ull << bits) - 1));
}

// status of a query (counts' companion array): != Q_OK marks inputs the reference leaves undefined
enum : uint8_t { Q_OK = 0, Q_EMPTY = 1, Q_SENTINEL = 2, Q_NON_ASCII = 3,
                 // class patterns only (mismatch_kernels.hip.h, CLASSES): a byte that is no class letter, more class positions than
                 // AWRY_MAX_CLASS_POSITIONS, a search abandoned at the expansion cap
                 Q_NOT_CLASS_LETTER = 4, Q_CLASS_POSITIONS = 5, Q_EXPANSION_CAP = 6 };

// Byte access through aligned 8-byte loads: one memory instruction per 8 consecutive bytes instead of one per byte
// (the lanes of a wave read different queries, so every byte load is a line lookup of its own in the texture path;
// the generic kernel's loops were bound by exactly that).  Reads the aligned word around a byte: the buffer must be
// readable up to the next 8-byte boundary (device allocations are).
struct ByteStream {
  const uint8_t* base;
  uint64_t word = 0;
  uintptr_t at = ~(uintptr_t)0;
  __device__ __forceinline__ explicit ByteStream(const uint8_t* p) : base(p) {}
  __device__ __forceinline__ uint8_t operator[](uint64_t i) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(base + i), w = a & ~(uintptr_t)7;
    if (w != at) { word = *reinterpret_cast<const uint64_t*>(w); at = w; }
    return (uint8_t)(word >> (8 * (a & 7)));
  }
};

// Eight ASCII nucleotide letters -> eight symbol indices, word-wise (src/alphabet.rs:109-114,169-248: A 1, C 2, G 3,
// T / U 5, everything else N = 4; '$' / '#' and bytes >= 0x80 never get here, their queries are rejected).
__device__ __forceinline__ uint64_t nt_indices8(uint64_t x) {
  constexpr uint64_t K7F = 0x7F7F7F7F7F7F7F7Full, K80 = 0x8080808080808080ull;
  const uint64_t c = x & 0xDFDFDFDFDFDFDFDFull;  // upper-case
  auto eq = [&](uint64_t pat) { const uint64_t t = c ^ pat; return (((((t & K7F) + K7F) | t) & K80) ^ K80) >> 7; };  // 1 per equal byte
  const uint64_t a = eq(0x4141414141414141ull), cc = eq(0x4343434343434343ull), g = eq(0x4747474747474747ull),
                 t = eq(0x5454545454545454ull) | eq(0x5555555555555555ull);
  return 0x0404040404040404ull - 3 * a - 2 * cc - g + t;  // bytewise, no borrows: at most one of the masks is set per byte
}

// Do the `rem` symbols text8[0 .. rem) equal the query bytes q[0 .. rem) (as symbol indices)?  Nucleotide: eight at a
// time; both buffers are readable 8 bytes past their end.
template <int A>
__device__ __forceinline__ bool text_equals_query(const uint8_t* __restrict__ text8, const uint8_t* __restrict__ q, uint64_t rem,
                                                  const uint8_t* lut) {
  if (A == NUCLEOTIDE) {
    for (uint64_t j = 0; j < rem; j += 8) {
      uint64_t tw, qw;
      __builtin_memcpy(&tw, text8 + j, 8);
      __builtin_memcpy(&qw, q + j, 8);
      uint64_t d = tw ^ nt_indices8(qw);
      if (rem - j < 8) d &= (1ull << (8 * (rem - j))) - 1;
      if (d) return false;
    }
    return true;
  }
  ByteStream t(text8), a(q);
  for (uint64_t j = 0; j < rem; j++)
    if (t[j] != lut[a[j]]) return false;
  return true;
}

}  // namespace awry
