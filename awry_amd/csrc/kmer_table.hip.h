// kmer_table.hip.h -- the kernels that build the k-mer count table (layout.h, KT_*) of one query length L from what is
// resident: the seed table, the keys and positions of the left-context index, the 4-bit text.  A part of kernels.hip.h:
// included there behind kernels_nt2_kmer.hip.h (needs lcx_text_letters of lcx.hip.h, LCX_LANE_ROWS), and not on its own.
//
// Why: a k-mer from a repeat family survives the probe pass with a seed bucket of 10^2..10^5 rows, and phase 2 then walks
// a chain of 4..6 dependent lines through the bucket's sorted keys.  The answer -- how many rows of the bucket have these
// L - k letters in front of them -- is a property of the index and of L alone, so it is worked out once, for every distinct
// L-mer of every such bucket, and kept: the lookup is one line (resume_block_list, mode 7).
#pragma once

namespace awry {

// adds n to the count of `key` (a 2L-bit query word) in its line: 64-bit compare-and-swap on the slots.  A key that finds
// its line full marks the line as overflowed; a count that leaves its field saturates at KT_ASK.  stats[0] += new entries,
// stats[1] += lines newly marked.
__device__ __forceinline__ void kt_add(uint64_t* __restrict__ table, uint32_t bits, uint64_t key, int L, uint64_t n, unsigned long long* __restrict__ stats) {
  const uint64_t mx = kt_mix(key, L);
  unsigned long long* line = reinterpret_cast<unsigned long long*>(table) + ((mx & ((1ull << bits) - 1)) << 4);
  const uint64_t tag = mx >> bits;
  // (a table forced smaller than its policy size, awry_debug_set_kmer_table_lines: a tag that does not fit its field is not kept)
  for (int u = tag >= KT_TAG_NONE ? 16 : 0; u < 16;) {
    const unsigned long long e = __hip_atomic_load(line + u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const uint64_t cnt = e & KT_CNT_MASK;
    if (cnt == 0) {  // an empty slot (slots never empty again, and fill before any line is marked)
      const uint64_t c = n < KT_ASK ? n : KT_ASK;
      if (atomicCAS(line + u, e, (tag << KT_TAG_SHIFT) | (e & KT_OVERFLOW) | c) == e) { atomicAdd(&stats[0], 1ull); return; }
      continue;  // somebody else took it: look at it again
    }
    if ((e >> KT_TAG_SHIFT) == tag) {
      const uint64_t c = cnt + n < KT_ASK ? cnt + n : KT_ASK;
      if (atomicCAS(line + u, e, (e & ~KT_CNT_MASK) | c) == e) return;
      continue;
    }
    u++;
  }
  if (!(atomicOr(line, (unsigned long long)KT_OVERFLOW) & KT_OVERFLOW)) atomicAdd(&stats[1], 1ull);
}

// One thread per BWT row r.  The suffix of row r names its seed bucket (its first k letters); a bucket phase 2 would search
// -- more than LCX_LANE_ROWS rows, in the left-context index -- is covered: slot r of the bucket holds one of its entries.
//   * a complete entry (its 32 left letters are ACGT; sorted by them) that is the first of its run of equal top 2 (L - k) key
//     bits finds the run's end by a galloping, then binary search of the keys and inserts (L-mer, run length);
//   * an incomplete entry (the bucket's last slots) whose nearest L - k left letters are nevertheless ACGT reads them from
//     the text and adds one to that L-mer.
// INSERT = false only counts what would be inserted (an upper bound on the entries: stats[2]), to size the table.
template <bool INSERT>
__global__ __launch_bounds__(256) void kt_scan_kernel(DevIndex ix, int L, uint64_t* __restrict__ table, uint32_t bits, unsigned long long* __restrict__ stats) {
  const int k = ix.seed_k, i0 = L - k, sh = 64 - 2 * i0;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  unsigned long long mine = 0;
  for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < ix.bwt_len; r += stride) {
    const uint32_t p = ix.dense_sa[r];
    bool ok = false;
    const uint64_t kmer = lcx_text_letters(ix.text4, p, k, &ok);
    if (!ok) continue;
    const SeedEntry e = ix.seed[kmer];
    if (seed_has_ctx(e) || (e.cnt & SEED_LCX_NONE)) continue;
    const uint32_t cnt = e.cnt & SEED_CNT_SAT;
    if (cnt <= (uint32_t)LCX_LANE_ROWS || cnt == SEED_CNT_SAT) continue;
    const uint32_t sp = e.sp, j = (uint32_t)r - sp;
    if (r < sp || j >= cnt) continue;  // (cannot happen: the rows of a bucket are the rows of its k-mer)
    const uint32_t inc = (e.cnt & SEED_LCX_TAIL) ? (uint32_t)ix.lcx_key[sp + cnt - 1u] : 0u;
    const uint32_t nc = cnt - (inc < cnt ? inc : cnt);
    if (j < nc) {
      const uint64_t ctx = ix.lcx_key[r] >> sh;
      if (j > 0 && (ix.lcx_key[r - 1] >> sh) == ctx) continue;  // not the first entry of its run
      if (!INSERT) { mine++; continue; }
      // the run's end: the first slot in (r, sp + nc] whose key differs
      const uint64_t end = (uint64_t)sp + nc;
      uint64_t lo = r, step = 1;  // key[lo] is in the run
      uint64_t hi = end;          // key[hi] is not (or hi == end)
      while (lo + step < end) {
        if ((ix.lcx_key[lo + step] >> sh) != ctx) { hi = lo + step; break; }
        lo += step;
        step <<= 1;
      }
      while (hi - lo > 1) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if ((ix.lcx_key[mid] >> sh) == ctx) lo = mid; else hi = mid;
      }
      kt_add(table, bits, ctx | (kmer << (2 * i0)), L, hi - r, stats);
    } else {
      const uint32_t tp = (uint32_t)ix.lcx_rowpos[r];
      if (tp < (uint32_t)i0) continue;  // the suffix starts too close to the text's beginning
      bool cok = false;
      const uint64_t ctx = lcx_text_letters(ix.text4, (uint64_t)tp - (uint64_t)i0, i0, &cok);
      if (!cok) continue;
      if (!INSERT) { mine++; continue; }
      kt_add(table, bits, ctx | (kmer << (2 * i0)), L, 1, stats);
    }
  }
  if (!INSERT && mine) atomicAdd(&stats[2], mine);
}

}  // namespace awry
