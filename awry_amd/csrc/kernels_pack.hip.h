// kernels_pack.hip.h -- the packer: ASCII nucleotide queries -> 2-bit words.
// A part of kernels.hip.h (one header, cut by kernel family): included there, in order, and not on its own.
#pragma once

namespace awry {

// ASCII queries -> packed words (letter j of a query in word j / 32, bits 2 (j % 32); W words per query, unused ones
// zero); *bad counts queries with a byte outside ACGTacgt and bad_list (if given, room for n entries) names them, in
// no particular order (U counts too: the caller redoes those queries with the generic kernel, which applies the full
// alphabet map).  RAGGED: query q is ascii[off[q] - base, off[q + 1] - base) and its length goes to
// lens[q]; otherwise every query has L bytes.
//
// A wave packs 64 consecutive queries at a time: their bytes are one contiguous range, fetched with coalesced 16-B
// loads into the wave's LDS tile, from which every lane packs its own query (one query per lane reading its bytes
// straight from global memory ran at 98 GB/s of ASCII).  Ranges that do not fit the tile are cut into fewer queries
// per pass; a single query longer than the tile is packed from global memory by its lane.
constexpr int PACK_TILE = 8192;  // bytes of LDS per wave
template <bool RAGGED>
__global__ __launch_bounds__(256) void pack_nt2_tile_kernel(const uint8_t* __restrict__ ascii, const uint64_t* __restrict__ off, uint64_t base,
                                                            uint64_t n, uint64_t total_bytes, int L, int W, uint64_t* __restrict__ words,
                                                            uint32_t* __restrict__ lens, unsigned long long* __restrict__ bad,
                                                            uint32_t* __restrict__ bad_list) {
  const int64_t mis = (int64_t)(reinterpret_cast<uintptr_t>(ascii) & 15);  // tile chunks are 16-B aligned in memory
  __shared__ __attribute__((aligned(16))) uint8_t s_tile[4][PACK_TILE + 16];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  uint8_t* tile = s_tile[wv];
  const uint64_t nwaves = (uint64_t)gridDim.x * 4, wave0 = (uint64_t)blockIdx.x * 4 + wv;
  for (uint64_t q0 = wave0 * 64; q0 < n; q0 += nwaves * 64) {  // wave-uniform trip count
    const uint64_t q = q0 + lane;
    const bool have = q < n;
    uint64_t s = 0, e = 0;  // this lane's query: bytes [s, e) of ascii
    if (have) {
      s = RAGGED ? off[q] - base : q * (uint64_t)L;
      e = RAGGED ? off[q + 1] - base : s + (uint64_t)L;
    }
    uint64_t done = 0;  // lanes [0, done) of this group of 64 are packed
    const uint64_t nq = n - q0 < 64 ? n - q0 : 64;
    while (done < nq) {
      // the longest run of queries starting at lane `done` whose bytes fit the tile (measured from a 16-B aligned start)
      const int64_t b0 = (int64_t)__shfl(s, (int)done, 64), a0 = ((b0 + mis) & ~15ll) - mis;  // may be < 0 by up to 15
      const bool fits = have && (uint64_t)lane >= done && (int64_t)e - a0 <= (int64_t)PACK_TILE;
      const uint64_t fm = __ballot(fits) >> done;
      const int m = fm == ~0ull ? 64 : __builtin_ctzll(~fm);  // leading run of fitting lanes
      const bool mine = (uint64_t)lane >= done && (uint64_t)lane < done + (m ? m : 1);
      auto pack_from = [&](auto src) {  // src: this lane's query bytes, in LDS or in global memory
        // eight letters per step, word-wise: upper-case, check that every byte is one of A C G T, take bits 1..2 of the
        // ASCII code (A 00, C 01, T 10, G 11), swap the last two, squeeze the eight 2-bit codes into 16 bits
        const int len = (int)(e - s);
        uint64_t w = 0;
        uint64_t ok = 0x8080808080808080ull;  // bit 7 of byte b stays set while letter b of every step was valid
        uint64_t* out = words + q * (uint64_t)W;
        constexpr uint64_t K7F = 0x7F7F7F7F7F7F7F7Full, K80 = 0x8080808080808080ull;
        auto eq = [&](uint64_t u, uint64_t pat) { const uint64_t t = u ^ pat; return ((((t & K7F) + K7F) | t) & K80) ^ K80; };
        for (int j = 0; j < len; j += 8) {
          const int nb = len - j < 8 ? len - j : 8;
          uint64_t x = 0;
          if (nb == 8) {
            __builtin_memcpy(&x, &src[j], 8);
          } else {
            for (int t = 0; t < nb; t++) x |= (uint64_t)src[j + t] << (8 * t);
            x |= 0x4141414141414141ull << (8 * nb);  // pad with 'A': valid, and zero bits in the packed word
          }
          const uint64_t c = x & 0xDFDFDFDFDFDFDFDFull;  // upper-case
          const uint64_t valid = (eq(c, 0x4141414141414141ull) | eq(c, 0x4343434343434343ull) | eq(c, 0x4747474747474747ull) |
                                  eq(c, 0x5454545454545454ull)) & ~(x & K80);  // and no byte >= 0x80 before the case fold
          ok &= valid;
          uint64_t y = (c >> 1) & 0x0303030303030303ull;
          y ^= (y >> 1) & 0x0101010101010101ull;
          y = (y | (y >> 6)) & 0x000F000F000F000Full;
          y = (y | (y >> 12)) & 0x000000FF000000FFull;
          y = (y | (y >> 24)) & 0xFFFFull;
          w |= y << (2 * (j & 31));
          if ((j & 31) == 24 || j + 8 >= len) { out[j >> 5] = w; w = 0; }
        }
        for (int k2 = (len + 31) >> 5; k2 < W; k2++) out[k2] = 0;
        if (RAGGED) lens[q] = (uint32_t)len;
        if (ok != K80) {  // rare: the caller redoes this query with the generic kernel
          const unsigned long long at = atomicAdd(bad, 1ull);
          if (bad_list) bad_list[at] = (uint32_t)q;
        }
      };
      if (m > 0) {
        const int64_t b1 = (int64_t)__shfl(e, (int)(done + m - 1), 64);
        for (int64_t i = a0 + 16ll * lane; i < b1; i += 16ll * 64) {
          if (i >= 0 && i + 16 <= (int64_t)total_bytes) {
            *reinterpret_cast<uint4*>(tile + (i - a0)) = *reinterpret_cast<const uint4*>(ascii + i);
          } else {  // first / last chunk of the buffer: only the bytes that exist
            for (int t = 0; t < 16; t++)
              if (i + t >= 0 && i + t < (int64_t)total_bytes) tile[i - a0 + t] = ascii[i + t];
          }
        }
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        if (mine && have) pack_from(tile + ((int64_t)s - a0));
      } else if (mine && have) {
        pack_from(ascii + s);  // one query longer than the tile: its lane reads global memory directly
      }
      __builtin_amdgcn_wave_barrier();
      done += m ? m : 1;
    }
  }
}

}  // namespace awry
