// kernels_count.hip.h -- generic count (one ASCII query per lane), the scalar conveniences and the reference's k-mer table.
// A part of kernels.hip.h (one header, cut by kernel family): included there, in order, and not on its own.
#pragma once

namespace awry {

// ------------------------------------------------------------------------------------------------
// generic count: one ASCII query per lane (any alphabet / symbol / length)
// ------------------------------------------------------------------------------------------------

// status[q] != 0 marks inputs the reference leaves undefined: empty query, '$'/'#',
// bytes >= 0x80.  ranges (optional) receives the final (start, end) row interval.
// allow_verify (with the dense SA and ix.text8 resident): once the range has shrunk to <= 4 rows, the letters still to
// the left are compared with the text in front of each candidate instead of being stepped one by one; ranges[2q] then
// holds an RS_SINGLE / RS_MULTI word for the locate pass, not a row interval -- callers that need rows pass 0.
// ulen != 0: every query has ulen bytes, back to back (off is not read).
// LIST_BLOCK: only the queries block b of an earlier pass (same grid) listed for itself, ql.q[b * ql.cap ...) -- the
// second phase of count_aa_kmer_probe_kernel.  LIST_GLOBAL: only the *ql.total queries of one device-wide list, in any
// order -- the reads of a packed nucleotide chunk that hold letters outside ACGT, redone in place; the first query
// (lowest index) with a non-zero status is reported through ql.first_bad as (index << 8 | status).
// LIST_COMPACT: the ql.cap listed queries travel as a CSR batch of their own -- entry `it` is bytes [off[it], off[it + 1])
// of ascii and answers for query ql.q[it] -- the form in which the host-packed paths hand over the few queries of a
// chunk that hold letters outside ACGT (only those bytes cross PCIe); first_bad as for LIST_GLOBAL.
enum { LIST_NONE = 0, LIST_BLOCK = 1, LIST_GLOBAL = 2, LIST_COMPACT = 3 };
struct QueryList {
  uint32_t* q;                      // query indices; LIST_BLOCK: block b owns slots [b * cap, (b + 1) * cap)
  uint32_t* count;                  // LIST_BLOCK: listed queries per block
  uint64_t cap;
  const unsigned long long* total;  // LIST_GLOBAL: number of listed queries
  unsigned long long* first_bad;    // LIST_GLOBAL (nullable): min over rejected queries of (index << 8 | status)
  uint32_t range_stride;            // LIST_GLOBAL: 1 = ranges[q] receives the range start / RS_* word only (the layout of
                                    //   the packed read kernels' range_start), otherwise (start, end) pairs
  unsigned long long* tally;        // nullable work census (untimed runs): [0] seed probes, [1] executed steps, [2] distinct
                                    //   blocks ranked, [3] SA reads and [4] text comparisons of seed-and-verify
  uint32_t nlists;                  // LIST_BLOCK: number of per-block lists (the first pass's grid), <= LIST_MAX_LISTS: the
                                    //   lists are then worked through as ONE pool by whatever grid this pass is launched
                                    //   with (0: block b takes list b)
};
__device__ __forceinline__ void tally_add(unsigned long long* tally, int slot, unsigned long long v) {
  if (tally && v) atomicAdd(&tally[slot], v);
}

template <int A, int LIST = LIST_NONE>
__global__ __launch_bounds__(256) void count_scalar_kernel(DevIndex ix, const uint8_t* __restrict__ ascii,
                                                           const uint64_t* __restrict__ off, uint64_t n,
                                                           uint64_t* __restrict__ counts, uint64_t* __restrict__ ranges,
                                                           uint8_t* __restrict__ status, int allow_verify, uint64_t ulen, QueryList ql) {
  __shared__ uint8_t lut[256];
  // LIST_BLOCK with ql.nlists: exclusive prefix sums of the lists' lengths.  The kernel holds ~140 VGPRs (3 waves per
  // SIMD), so a grid of one block per list ran in three rounds, each as long as the longest chain of dependent loads in
  // it -- 66 us for a few hundred thousand queries; as one pool the listed queries spread over every resident thread.
  __shared__ uint32_t s_pref[LIST == LIST_BLOCK ? LIST_MAX_LISTS + 1 : 1];
  lut[threadIdx.x] = (uint8_t)(threadIdx.x >= 128 ? 0xFF : index_of_ascii(A, (uint8_t)threadIdx.x));
  const bool pooled = LIST == LIST_BLOCK && ql.nlists != 0;
  uint64_t pool_total = 0;
  if (LIST == LIST_BLOCK && pooled) {
    const uint32_t per = (ql.nlists + blockDim.x - 1) / blockDim.x;  // consecutive lists per thread
    const uint32_t l0 = threadIdx.x * per;
    uint64_t mine = 0;
    for (uint32_t j = 0; j < per; j++) mine += l0 + j < ql.nlists ? ql.count[l0 + j] : 0u;
    uint64_t tot;
    uint64_t run = block_excl_scan(mine, &tot);
    for (uint32_t j = 0; j < per; j++)
      if (l0 + j < ql.nlists) { s_pref[l0 + j] = (uint32_t)run; run += ql.count[l0 + j]; }
    if (threadIdx.x == 0) s_pref[ql.nlists] = (uint32_t)tot;
    pool_total = tot;
  }
  __syncthreads();
  const uint64_t stride = LIST == LIST_BLOCK && !pooled ? blockDim.x : (uint64_t)gridDim.x * blockDim.x;
  const uint64_t todo = LIST == LIST_BLOCK ? (pooled ? pool_total : (uint64_t)ql.count[blockIdx.x])
                                           : (LIST == LIST_GLOBAL ? (uint64_t)*ql.total : (LIST == LIST_COMPACT ? ql.cap : n));
  const uint8_t* const ascii_bytes = ascii;
  for (uint64_t it = LIST == LIST_BLOCK && !pooled ? threadIdx.x : (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; it < todo; it += stride) {
    uint64_t q;
    if (LIST == LIST_BLOCK && pooled) {  // item `it` of the pool: list l with s_pref[l] <= it < s_pref[l + 1]
      uint32_t lo = 0, hi = ql.nlists;
      while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (s_pref[mid] <= (uint32_t)it) lo = mid; else hi = mid; }
      q = ql.q[(uint64_t)lo * ql.cap + (it - s_pref[lo])];
    } else {
      q = LIST == LIST_BLOCK ? ql.q[(uint64_t)blockIdx.x * ql.cap + it] : (LIST == LIST_GLOBAL || LIST == LIST_COMPACT ? ql.q[it] : it);
    }
    const uint64_t b = LIST == LIST_COMPACT ? off[it] : (ulen ? q * ulen : off[q]);
    const uint64_t e = LIST == LIST_COMPACT ? off[it + 1] : (ulen ? b + ulen : off[q + 1]);
    ByteStream ascii(ascii_bytes);  // shadows the pointer: same indexing, 8 bytes per load
    uint8_t st = e > b ? Q_OK : Q_EMPTY;
    if (A == NUCLEOTIDE) {  // eight bytes at a time: any byte >= 0x80, any '$' or '#'
      constexpr uint64_t K7F = 0x7F7F7F7F7F7F7F7Full, K80 = 0x8080808080808080ull;
      uint64_t high = 0, sent = 0;
      for (uint64_t i = b; i < e; i += 8) {
        uint64_t x;
        __builtin_memcpy(&x, ascii_bytes + i, 8);
        if (e - i < 8) x &= (1ull << (8 * (e - i))) - 1;  // bytes past the query read as 0: neither test fires
        high |= x & K80;
        const uint64_t t1 = x ^ 0x2424242424242424ull, t2 = x ^ 0x2323232323232323ull;
        sent |= (((((t1 & K7F) + K7F) | t1) & K80) ^ K80) | (((((t2 & K7F) + K7F) | t2) & K80) ^ K80);
      }
      if (high) st = Q_NON_ASCII;
      else if (sent && st == Q_OK) st = Q_SENTINEL;
    } else {
      for (uint64_t i = b; i < e; i++) {
        uint8_t s = lut[ascii[i]];
        if (s == 0xFF) st = Q_NON_ASCII;
        else if (s == 0 && st == Q_OK) st = Q_SENTINEL;
      }
    }
    uint64_t sp = 1, ep = 0, vcount = 0, vrs = 0;
    bool verified = false;
    if (st == Q_OK) {
      uint64_t i = e - 1;
      bool seeded = false;
      // reference schedule (awry_search_range): no table, and kmer_len - 1 steps taken whether or not the range is empty
      // (src/kmer_lookup_table.rs:90-110), so that the rows of an ABSENT query are the reference's too
      const bool ref_mode = (allow_verify & 2) != 0;
      uint64_t uncond = ref_mode && e - b >= (uint64_t)(allow_verify >> 8) && (allow_verify >> 8) > 0 ? (uint64_t)(allow_verify >> 8) - 1 : 0;
      if (ref_mode) allow_verify = 0;
      if (!ref_mode && A == AMINO && ix.seed && e - b >= (uint64_t)ix.seed_k) {  // last k residues all standard -> one table probe
        const int k = ix.seed_k;
        uint64_t sidx = 0;
        bool std20 = true;
        for (int j = k - 1; j >= 0; j--) {  // leftmost window letter least significant
          const int letter = aa_letter_of_index(lut[ascii[e - k + j]]);
          std20 = std20 && letter >= 0;
          sidx = sidx * AA_SEED_SIGMA + (uint64_t)(letter < 0 ? 0 : letter);
        }
        if (std20) {
          const SeedEntry se = seed_probe(ix.seed + sidx);
          tally_add(ql.tally, 0, 1);
          const uint32_t scnt = aa_seed_cnt(se);
          // BWT[row] is not the next residue / the next residue does not occur in the BWT over the entry's 2..4 rows
          const bool wrong_sym = e - k > b && ((scnt == 1 && (int)aa_seed_sym(se) != (int)lut[ascii[e - k - 1]]) ||
                                               (aa_seed_is_multi(se) && !((aa_seed_mask(se) >> lut[ascii[e - k - 1]]) & 1u)));
          if (ix.seed_pos && scnt == 1 && !wrong_sym) {  // position seed, as in the nucleotide branch below
            const uint64_t rem = e - k - b, p = se.sp;
            if (allow_verify && ix.text8 && rem < 65536) {
              const bool same = p >= rem && text_equals_query<A>(ix.text8 + (p - rem), ascii_bytes + b, rem, lut);
              tally_add(ql.tally, 4, p >= rem ? 1 : 0);
              verified = true;
              vcount = same ? 1 : 0;
              vrs = same ? ((RS_SINGLE << RS_MODE_SHIFT) | (p - rem)) : ((RS_MULTI << RS_MODE_SHIFT) | (rem << 32));
              seeded = true;
              sp = 1; ep = 0;
            }
          } else if (scnt != AA_SEED_CNT_SAT) {
            sp = scnt ? se.sp : 1;
            ep = scnt ? (uint64_t)se.sp + scnt - 1 : 0;
            i = e - k;
            seeded = true;
            if (wrong_sym) { sp = 1; ep = 0; }
          }
        }
      }
      if (!ref_mode && A == NUCLEOTIDE && ix.seed && e - b >= (uint64_t)ix.seed_k) {  // last k symbols all in ACGT -> one table probe
        const int k = ix.seed_k;
        uint64_t sidx = 0;
        bool acgt = true;
        for (int j = 0; j < k; j++) {
          const int letter = nt_letter_of_index(lut[ascii[e - k + j]]);
          acgt = acgt && letter >= 0;
          sidx |= (uint64_t)(letter & 3) << (2 * j);  // leftmost letter of the window least significant
        }
        if (acgt) {
          const SeedEntry se = seed_probe(ix.seed + sidx);
          tally_add(ql.tally, 0, 1);
          const uint32_t scnt = seed_cnt(se);
          const bool wrong_sym = scnt == 1 && e - k > b && seed_sym(se) != (int)lut[ascii[e - k - 1]];  // BWT[row] is not the next symbol
          // position seeds (ix.seed_pos): a singleton entry names a text position, not a row -- good enough to reject
          // the query by its symbol or to finish it against the text, not to continue the search: without the text
          // such a query starts over without the table
          if (ix.seed_pos && scnt == 1 && !wrong_sym) {
            const uint64_t rem = e - k - b, p = seed_position(se, (int)ix.ctx_extra);
            if (allow_verify && ix.text8 && rem < 65536) {
              // (p < rem: the suffix starts too close to the text's beginning)
              const bool same = p >= rem && text_equals_query<A>(ix.text8 + (p - rem), ascii_bytes + b, rem, lut);
              tally_add(ql.tally, 4, p >= rem ? 1 : 0);
              verified = true;
              vcount = same ? 1 : 0;
              vrs = same ? ((RS_SINGLE << RS_MODE_SHIFT) | (p - rem)) : ((RS_MULTI << RS_MODE_SHIFT) | (rem << 32));
              seeded = true;
              sp = 1; ep = 0;  // skips the step loop below
            }
          } else if (scnt != SEED_CNT_SAT) {
            sp = scnt ? se.sp : 1;
            ep = scnt ? (uint64_t)se.sp + scnt - 1 : 0;
            i = e - k;
            seeded = true;
            if (wrong_sym) { sp = 1; ep = 0; }
          }
        }
      }
      if (!seeded) {
        int idx = lut[ascii[i]];
        sp = ix.prefix_sums[idx];          // SearchRange::new, src/search.rs:43-48
        ep = ix.prefix_sums[idx + 1] - 1;
      }
      const bool can_verify = allow_verify && ix.text8 && ix.dense_sa && ix.dense_ratio == 1;
      while (i > b && (sp <= ep || uncond > 0)) {  // emptiness is sticky, so stopping early never changes the count
        if (uncond > 0) uncond--;
        const uint64_t rem = i - b, cnt = ep - sp + 1;
        // (second pass of the amino k-mer schedule: what counts there is the length of the chain of dependent loads, and
        //  SA + text is two of them where every LF step is one more)
        if (can_verify && cnt <= 4 && (3 * cnt <= rem || LIST == LIST_BLOCK) && rem < 65536) {
          uint32_t mask = 0;
          uint64_t g1 = 0;
          if (A == AMINO && rem <= 24) {
            // short rests (k-mers): the candidates' SA entries, then their text words, are fetched TOGETHER -- two or three
            // dependent round trips for up to four candidates instead of two or three per candidate
            uint32_t pc[4];
#pragma unroll
            for (int c = 0; c < 4; c++) pc[c] = (uint64_t)c < cnt ? ix.dense_sa[sp + c] : 0u;
            uint64_t diff[4] = {0, 0, 0, 0};
            for (uint64_t w0 = 0; w0 < rem; w0 += 8) {
              const int nb = rem - w0 < 8 ? (int)(rem - w0) : 8;
              uint64_t qw = 0;
              for (int t = 0; t < nb; t++) qw |= (uint64_t)lut[ascii[b + w0 + t]] << (8 * t);
              const uint64_t m = nb >= 8 ? ~0ull : (1ull << (8 * nb)) - 1;
              uint64_t tw[4];
#pragma unroll
              for (int c = 0; c < 4; c++) {
                tw[c] = ~qw;
                if ((uint64_t)c < cnt && pc[c] >= rem) __builtin_memcpy(&tw[c], ix.text8 + ((uint64_t)pc[c] - rem) + w0, 8);  // (16 bytes of slack behind the text)
              }
#pragma unroll
              for (int c = 0; c < 4; c++) diff[c] |= (tw[c] ^ qw) & m;
            }
#pragma unroll
            for (int c = 0; c < 4; c++)
              if ((uint64_t)c < cnt) {
                tally_add(ql.tally, 3, 1);
                if (pc[c] >= rem) {
                  tally_add(ql.tally, 4, 1);
                  if (!diff[c]) { mask |= 1u << c; g1 = (uint64_t)pc[c] - rem; }
                }
              }
          } else
          for (uint64_t c = 0; c < cnt; c++) {
            const uint64_t p = ix.dense_sa[sp + c];
            tally_add(ql.tally, 3, 1);
            if (p < rem) continue;  // the suffix starts too close to the text's beginning
            tally_add(ql.tally, 4, 1);
            if (text_equals_query<A>(ix.text8 + (p - rem), ascii_bytes + b, rem, lut)) { mask |= 1u << c; g1 = p - rem; }
          }
          verified = true;
          vcount = (uint64_t)__popc(mask);
          vrs = (cnt == 1 && mask) ? ((RS_SINGLE << RS_MODE_SHIFT) | g1)
                                   : ((RS_MULTI << RS_MODE_SHIFT) | sp | (rem << 32) | ((uint64_t)mask << 48));
          break;
        }
        i--;
        if (ql.tally) { tally_add(ql.tally, 1, 1); tally_add(ql.tally, 2, ((sp - 1) >> 8) == (ep >> 8) ? 1 : 2); }
        step_scalar<A>(ix, sp, ep, lut[ascii[i]]);
      }
    }
    const bool starts_only = (LIST == LIST_GLOBAL || LIST == LIST_COMPACT) && ql.range_stride == 1;
    if (verified) {
      counts[q] = vcount;
      if (ranges) { if (starts_only) ranges[q] = vrs; else { ranges[2 * q] = vrs; ranges[2 * q + 1] = 0; } }
    } else {
      counts[q] = sp > ep ? 0 : ep - sp + 1;  // src/search.rs:66-71
      if (ranges) { if (starts_only) ranges[q] = sp; else { ranges[2 * q] = sp; ranges[2 * q + 1] = ep; } }
    }
    if (status) status[q] = st;
    if ((LIST == LIST_GLOBAL || LIST == LIST_COMPACT) && ql.first_bad && st != Q_OK) atomicMin(ql.first_bad, ((unsigned long long)q << 8) | st);
  }
}

// one step / one backstep / one initial range for the scalar conveniences of the C ABI
template <int A>
__global__ void scalar_ops_kernel(DevIndex ix, int op, uint64_t a, uint64_t b, int idx, uint64_t* out) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  if (op == 0) {  // update_range_with_symbol
    uint64_t sp = a, ep = b;
    step_scalar<A>(ix, sp, ep, idx);
    out[0] = sp; out[1] = ep;
  } else if (op == 1) {  // backstep
    out[0] = backstep_scalar<A>(ix, a);
  } else if (op == 2) {  // global_occurrence
    out[0] = rank_scalar<A>(ix, a, idx);
  } else {  // symbol_at
    out[0] = (uint64_t)symbol_at<A>(ix, a);
  }
}

// ------------------------------------------------------------------------------------------------
// the reference's k-mer table content, for byte-identical .awry files (src/kmer_lookup_table.rs:121-167):
// slot = sum_j s_j * sigma^j with s_0 = LAST symbol, digits restricted to 1..sigma-1; steps are applied
// without any emptiness check; every other slot stays SearchRange::zero() = {1, 0}.
// ------------------------------------------------------------------------------------------------
template <int A>
__global__ __launch_bounds__(256) void ref_kmer_table_kernel(DevIndex ix, int kmer_len, uint64_t nslots,
                                                             uint64_t* __restrict__ table) {
  const uint64_t sigma = A == NUCLEOTIDE ? 4 : 20;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t slot = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; slot < nslots; slot += stride) {
    uint64_t sp = 1, ep = 0, rem = slot;
    bool populated = kmer_len > 0;
    for (int j = 0; j < kmer_len; j++) {
      if (rem % sigma == 0) populated = false;
      rem /= sigma;
    }
    if (populated) {
      rem = slot;
      int idx = (int)(rem % sigma);
      rem /= sigma;
      sp = ix.prefix_sums[idx];
      ep = ix.prefix_sums[idx + 1] - 1;
      for (int j = 1; j < kmer_len; j++) {
        idx = (int)(rem % sigma);
        rem /= sigma;
        step_scalar<A>(ix, sp, ep, idx);
      }
    }
    table[2 * slot] = sp;
    table[2 * slot + 1] = ep;
  }
}

}  // namespace awry
