// kernels_aa_kmer.hip.h -- amino k-mer batches: the probe pass in front of count_scalar_kernel<AMINO, LIST_BLOCK>.
// A part of kernels.hip.h (one header, cut by kernel family): included there, in order, and not on its own.
#pragma once

namespace awry {

// ------------------------------------------------------------------------------------------------
// Amino k-mer batches: n ASCII queries of the same length L (AA_KMER_MIN..AA_KMER_MAX residues) back to back -- the
// shape of BASELINE configs[3] (10 M 12-mers).  First phase of a two-phase schedule, one query per LANE, NQ in flight:
// the bytes of a query are two or three unaligned 8-byte loads at q * L (no offsets, no byte stream), an LDS table
// turns each byte into its symbol index and its base-20 digit, the last k residues name one seed entry (the query's
// one random line).  Entry empty: absent.  Singleton whose BWT symbol is not the next residue: absent.  Singleton
// otherwise (position seeds, dense SA and byte text resident): the L - k residues in front of the one candidate are
// one <= 24-B window of the text, compared word-wise; an entry of 2..AA_KMER_VMULTI rows likewise, candidate by
// candidate through the dense SA, when enough lanes of the wave hold one.  Everything else -- a non-standard residue
// in the seed window, bytes the reference leaves undefined, entries with more rows, row seeds -- is listed per block
// and redone by count_scalar_kernel<AMINO, LIST_BLOCK> on the same grid.  The generic kernel spends ~1 900 wave instructions
// per 64 such queries, most of them offset and byte-stream bookkeeping; this pass executes 300-400 (counted in the ISA for L = 12).
// ranges (optional): what the locate pass reads for a settled query, in the generic kernel's layout -- ranges[2q] = a row
// interval's start or an RS_SINGLE / RS_MULTI word (verified text position / candidate rows + mask), ranges[2q + 1] = 0.
constexpr int AA_KMER_MIN = 8, AA_KMER_MAX = 24;
// LONG: queries of up to AA_KMER_LONG_MAX residues (peptides, protein fragments).  The pass works on a query's LAST 24
// residues exactly as above -- seed window, the residue in front of it, up to 17 residues compared in registers -- and the
// residues before those (the "far" part) are screened for bytes the reference leaves undefined when the query is loaded and
// compared with the text, eight at a time, only for candidates that passed everything else.  (The generic kernel serves a
// 40-residue batch from the text at 3.9 G queries/s; this pass at the rate of its 24-residue tail plus that comparison.)
constexpr int AA_KMER_LONG_MAX = 1024;
// symbol index of residue j of a query held as three words of one index per byte
__device__ __forceinline__ uint32_t jn_idx(uint64_t i0, uint64_t i1, uint64_t i2, int j) {
  const uint64_t w = j < 8 ? i0 : (j < 16 ? i1 : i2);
  return (uint32_t)((w >> (8 * (j & 7))) & 0xFF);
}
constexpr int AA_KMER_VMULTI = 4;        // seed ranges of up to this many rows are verified candidate by candidate
constexpr int AA_KMER_VMULTI_LANES = 8;  //   when at least this many lanes of the wave hold one (1 and 3 measure no better)

// RAGGED: query q is ascii[off[q], off[q + 1]) with its own length (k .. AA_KMER_MAX residues take this pass, any other
// length is listed for the generic kernel); L is then ignored.  Same per-lane work with the length, the number of
// residues left of the seed window and the byte masks as per-lane values instead of wave constants.
template <int NQ, bool RAGGED = false, bool LONG = false>
__global__ __launch_bounds__(256) void count_aa_kmer_probe_kernel(DevIndex ix, const uint8_t* __restrict__ ascii, const uint64_t* __restrict__ off,
                                                                  uint64_t n, int L, uint64_t* __restrict__ counts, uint64_t* __restrict__ ranges,
                                                                  uint8_t* __restrict__ status, QueryList ql) {
  // per byte: bits 0..4 symbol index, bits 8..12 digit of the seed-table index (the 21 searchable symbols), bit 15
  // undefined in the reference ('$', '#', bytes >= 0x80)
  __shared__ uint16_t lut[256];
  __shared__ unsigned int s_count;
  {
    const int c = threadIdx.x;
    const int idx = c >= 128 ? 0 : index_of_ascii(AMINO, (uint8_t)c);
    const int digit = aa_letter_of_index(idx);
    lut[c] = (uint16_t)(idx <= 0 ? 0x8000 : (idx | (digit < 0 ? 0x4000 : digit << 8)));
  }
  if (threadIdx.x == 0) s_count = 0;
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int k = ix.seed_k;
  const SeedEntry* __restrict__ seed = ix.seed;
  const bool pos = ix.seed_pos && ix.text8 && ix.dense_sa && ix.dense_ratio == 1;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  const uint64_t lane_lt = (1ull << lane) - 1;
  const uint64_t region = (uint64_t)blockIdx.x * ql.cap;
  auto bytes_mask = [](int m) { return m >= 8 ? ~0ull : (m <= 0 ? 0ull : (1ull << (8 * m)) - 1); };
  auto ld8 = [](const uint8_t* p) { uint64_t v; __builtin_memcpy(&v, p, 8); return v; };
  // LONG: does a word hold a byte >= 0x80, a '$' or a '#' (the bytes whose symbol index is not positive)?
  auto undefined8 = [](uint64_t x) {
    constexpr uint64_t K7F = 0x7F7F7F7F7F7F7F7Full, K80 = 0x8080808080808080ull;
    const uint64_t t1 = x ^ 0x2424242424242424ull, t2 = x ^ 0x2323232323232323ull;
    return (x & K80) | (((((t1 & K7F) + K7F) | t1) & K80) ^ K80) | (((((t2 & K7F) + K7F) | t2) & K80) ^ K80);
  };
  // LONG: are the `far` residues at qp (ASCII) the symbols at text8[tpos, tpos + far)?
  auto far_equal = [&](uint64_t tpos, const uint8_t* qp, int far) {
    for (int w0 = 0; w0 < far; w0 += 8) {
      const uint64_t qc = ld8(qp + w0), tw = ld8(ix.text8 + tpos + (uint64_t)w0);  // (the query's 24-residue tail follows: in bounds)
      uint64_t iw = 0;
#pragma unroll
      for (int bj = 0; bj < 8; bj++) iw |= (uint64_t)(lut[(qc >> (8 * bj)) & 0xFF] & 0x1Fu) << (8 * bj);
      const int nb = far - w0;
      if ((tw ^ iw) & (nb >= 8 ? ~0ull : (1ull << (8 * nb)) - 1)) return false;
    }
    return true;
  };
  // which of the candidates at text positions p[0 .. nc) have the query's first `rem` residues in front of them (bit c)
  auto candidates = [&](const uint32_t (&p)[AA_KMER_VMULTI], uint32_t nc, uint64_t j0, uint64_t j1, uint64_t j2, int rem) {
    const uint64_t m0 = bytes_mask(rem), m1 = bytes_mask(rem - 8), m2 = bytes_mask(rem - 16);
    uint32_t found = 0;
#pragma unroll
    for (int c = 0; c < AA_KMER_VMULTI; c++) {
      if ((uint32_t)c >= nc || p[c] < (uint32_t)rem) continue;  // (the suffix starts too close to the text's beginning)
      const uint8_t* t = ix.text8 + ((uint64_t)p[c] - (uint64_t)rem);
      uint64_t d = (ld8(t) ^ j0) & m0;
      if (rem > 8) d |= (ld8(t + 8) ^ j1) & m1;
      if (rem > 16) d |= (ld8(t + 16) ^ j2) & m2;
      found |= d ? 0u : 1u << c;
    }
    return found;
  };
  // the trip count is wave-uniform (ballots and the wave-level atomic below need every lane of the wave)
  for (uint64_t wbase = (uint64_t)blockIdx.x * blockDim.x + (threadIdx.x & ~63u); wbase < n; wbase += NQ * stride) {
    uint64_t qv[NQ], c0[NQ], c1[NQ], c2[NQ];
    int Lq[NQ];      // residues of the query this pass holds in registers (LONG: its last 24; RAGGED: per query)
    int far[NQ];     // LONG: residues in front of those
    const uint8_t* qp[NQ];  // LONG: the query's first byte
    bool odd[NQ];    // RAGGED: length outside k .. AA_KMER_MAX (LONG: AA_KMER_LONG_MAX)
#pragma unroll
    for (int h = 0; h < NQ; h++) {  // bytes [0, 8), [8, 16), [16, 24) of the query (bytes past its end are ignored below)
      qv[h] = wbase + lane + (uint64_t)h * stride;
      c0[h] = c1[h] = c2[h] = 0;
      Lq[h] = LONG && L > AA_KMER_MAX ? AA_KMER_MAX : L;
      far[h] = 0;
      qp[h] = ascii;
      odd[h] = false;
      if (qv[h] < n) {
        if (RAGGED) {
          const uint64_t b = off[qv[h]], len = off[qv[h] + 1] - b;
          odd[h] = len < (uint64_t)(k > 1 ? k : 1) || len > (uint64_t)(LONG ? AA_KMER_LONG_MAX : AA_KMER_MAX);
          Lq[h] = odd[h] ? AA_KMER_MAX : (len > (uint64_t)AA_KMER_MAX ? AA_KMER_MAX : (int)len);
          if (!odd[h]) {  // never reads a byte past the query's last one (a caller's buffer may end right there)
            if (LONG) { far[h] = (int)len - Lq[h]; qp[h] = ascii + b; }
            const uint64_t first = b + (LONG ? (uint64_t)far[h] : 0ull);
            const uint8_t* p = ascii + first;
            const int Lt = Lq[h];
            if (Lt >= 8) {  // the last word is anchored at the query's end, as in the equal-length branch
              c0[h] = ld8(p);
              const uint64_t last = ld8(p + Lt - 8);
              if (Lt >= 16) { c1[h] = ld8(p + 8); if (Lt > 16) c2[h] = last >> (8 * (24 - Lt)); }
              else if (Lt > 8) c1[h] = last >> (8 * (16 - Lt));
            } else if (first + (uint64_t)Lt >= 8) {  // shorter than a word: the word that ENDS with the query
              c0[h] = ld8(p + Lt - 8) >> (8 * (8 - Lt));
            } else {  // within the buffer's first seven bytes
              for (int t = 0; t < Lt; t++) c0[h] |= (uint64_t)p[t] << (8 * t);
            }
          }
        } else {
          const int Lt = Lq[h];
          if (LONG) { far[h] = L - Lt; qp[h] = ascii + qv[h] * (uint64_t)L; }
          const uint8_t* p = ascii + qv[h] * (uint64_t)L + (LONG ? (uint64_t)far[h] : 0ull);
          c0[h] = ld8(p);
          if (Lt > 8) {
            const uint64_t last = ld8(p + Lt - 8);  // never reads past the query
            if (Lt >= 16) { c1[h] = ld8(p + 8); if (Lt > 16) c2[h] = last >> (8 * (24 - Lt)); }
            else c1[h] = last >> (8 * (16 - Lt));
          }
        }
      }
    }
    uint64_t i0[NQ], i1[NQ], i2[NQ];  // the same bytes as symbol indices
    uint32_t flags[NQ];
    SeedEntry ev[NQ];
#pragma unroll
    for (int h = 0; h < NQ; h++) {
      const int len = Lq[h], rem = len - k;
      uint32_t slot = 0, mul = 1, fl = odd[h] ? 0x4000u : 0u;  // 21^7 < 2^32
      auto word = [&](uint64_t c, int base) {
        uint64_t iw = 0;
#pragma unroll
        for (int bj = 0; bj < 8; bj++) {
          const int j = base + bj;
          if (j < len) {
            const uint32_t t = lut[(c >> (8 * bj)) & 0xFF];
            fl |= t & 0x8000u;
            iw |= (uint64_t)(t & 0x1Fu) << (8 * bj);
            if (j >= rem) {  // seed window: leftmost residue least significant
              fl |= t & 0x4000u;
              slot += ((t >> 8) & 0x1Fu) * mul;
              mul *= (uint32_t)AA_SEED_SIGMA;
            }
          }
        }
        return iw;
      };
      i0[h] = word(c0[h], 0);
      i1[h] = word(c1[h], 8);
      i2[h] = word(c2[h], 16);
      if (LONG && qv[h] < n && !odd[h]) {  // the far residues: any byte the reference leaves undefined sends the query to the generic kernel
        uint64_t und = 0;
        for (int w0 = 0; w0 < far[h]; w0 += 8) {
          uint64_t x = ld8(qp[h] + w0);
          if (far[h] - w0 < 8) x &= (1ull << (8 * (far[h] - w0))) - 1;
          und |= undefined8(x);
        }
        if (und) fl |= 0x8000u;
      }
      flags[h] = fl;
      ev[h] = SeedEntry{1u, 0u};
      if (qv[h] < n && !fl) ev[h] = seed_probe(seed + slot);
      if (ql.tally) { const uint64_t pm = __ballot(qv[h] < n && !fl); if (lane == 0) tally_add(ql.tally, 0, (unsigned long long)__popcll(pm)); }
    }
    bool listed[NQ], vfy[NQ], multi[NQ];
    uint64_t value[NQ], rs[NQ], t0[NQ], t1[NQ], t2[NQ];  // rs: what the locate pass reads for the query (ranges[2q])
#pragma unroll
    for (int h = 0; h < NQ; h++) {
      const SeedEntry e = ev[h];
      const uint32_t scnt = aa_seed_cnt(e);
      const int rem = Lq[h] - k;
      listed[h] = vfy[h] = multi[h] = false;
      value[h] = 0;
      rs[h] = (RS_PLAIN << RS_MODE_SHIFT) | 1ull;  // no hits
      t0[h] = t1[h] = t2[h] = 0;
      if (qv[h] >= n) continue;
      if (flags[h]) listed[h] = true;
      else if (scnt == 0u) value[h] = 0;
      else if (rem == 0) {  // the seed window is the whole query: the entry is the answer
        if (scnt == AA_SEED_CNT_SAT) listed[h] = true;
        else { value[h] = scnt; rs[h] = scnt == 1u && ix.seed_pos ? ((RS_SINGLE << RS_MODE_SHIFT) | e.sp) : ((RS_PLAIN << RS_MODE_SHIFT) | e.sp); }
      }
      else if (scnt == 1u) {
        // the residue in front of the seed window must be BWT[row]
        if (jn_idx(i0[h], i1[h], i2[h], rem - 1) != aa_seed_sym(e)) value[h] = 0;
        else if (aa_seed_is_ctx(e) && rem <= AA_SEED_CTX_LEN) {
          // the entry holds the residues in front of the one occurrence: decided here, no text access
          uint32_t qctx = 0;  // query residues rem-2, rem-3, ... 0 in the entry's order (rem <= 6: all in bytes 0..7)
#pragma unroll
          for (int j = 0; j < AA_SEED_CTX_LEN - 1; j++)
            if (j < rem - 1) qctx |= (uint32_t)((i0[h] >> (8 * (rem - 2 - j))) & 0x1Fu) << (5 * j);
          const uint32_t cmask = rem >= 2 ? (1u << (5 * (rem - 1))) - 1u : 0u;
          if ((aa_seed_ctx(e) & cmask) == qctx) { value[h] = 1; rs[h] = (RS_SINGLE << RS_MODE_SHIFT) | ((uint64_t)e.sp - (uint64_t)rem); }
        }
        else if (pos) {
          if (e.sp >= (uint32_t)(rem + (LONG ? far[h] : 0))) {  // else the suffix starts too close to the text's beginning
            vfy[h] = true;  // the window's loads are issued here, for all NQ queries, and compared below
            const uint8_t* t = ix.text8 + ((uint64_t)e.sp - (uint64_t)rem);
            t0[h] = ld8(t);
            if (rem > 8) t1[h] = ld8(t + 8);
            if (rem > 16) t2[h] = ld8(t + 16);
          }
        } else listed[h] = true;
      } else if (aa_seed_is_multi(e) && !((aa_seed_mask(e) >> (jn_idx(i0[h], i1[h], i2[h], rem - 1) & 0x1Fu)) & 1u)) {
        value[h] = 0;  // the residue in front of the seed window does not occur in the BWT over the entry's rows: absent
      } else if (pos && scnt <= (uint32_t)AA_KMER_VMULTI) multi[h] = true;
      else listed[h] = true;
    }
#pragma unroll
    for (int h = 0; h < NQ; h++) {
      const int rem = Lq[h] - k;
      if (vfy[h]) {
        value[h] = (((t0[h] ^ i0[h]) & bytes_mask(rem)) | ((t1[h] ^ i1[h]) & bytes_mask(rem - 8)) | ((t2[h] ^ i2[h]) & bytes_mask(rem - 16))) ? 0ull : 1ull;
        if (LONG && value[h] && far[h] > 0 && !far_equal((uint64_t)ev[h].sp - (uint64_t)rem - (uint64_t)far[h], qp[h], far[h])) value[h] = 0;
        if (value[h]) rs[h] = (RS_SINGLE << RS_MODE_SHIFT) | ((uint64_t)ev[h].sp - (uint64_t)rem - (uint64_t)(LONG ? far[h] : 0));
      }
      if (ql.tally) { const uint64_t vm = __ballot(vfy[h]); if (lane == 0) tally_add(ql.tally, 4, (unsigned long long)__popcll(vm)); }
      // A handful of candidate rows, neighbours in the dense SA: each is compared with the text -- two dependent loads
      // the whole wave waits for, so a wave does it only when enough of its lanes need it (a batch of k-mers from the
      // text); the odd such lane of a random batch is listed, and the second pass works through those densely.
      // (Queueing them in LDS until a wave-full is pending, as the nucleotide probe does, was measured: the work
      // moves from the second pass into this one and the sum grows by 6 %.)
      const uint64_t mm = __ballot(multi[h]);
      if (__popcll(mm) < AA_KMER_VMULTI_LANES) { listed[h] = listed[h] || multi[h]; multi[h] = false; }
      if (multi[h]) {
        const uint32_t sp = ev[h].sp, nc = aa_seed_cnt(ev[h]);
        uint32_t p[AA_KMER_VMULTI];
#pragma unroll
        for (int c = 0; c < AA_KMER_VMULTI; c++) p[c] = (uint32_t)c < nc ? ix.dense_sa[sp + c] : 0u;
        uint32_t mask = candidates(p, nc, i0[h], i1[h], i2[h], rem);
        if (LONG && far[h] > 0) {
#pragma unroll
          for (int c = 0; c < AA_KMER_VMULTI; c++)
            if ((mask >> c) & 1u)
              if (p[c] < (uint32_t)(rem + far[h]) || !far_equal((uint64_t)p[c] - (uint64_t)rem - (uint64_t)far[h], qp[h], far[h])) mask &= ~(1u << c);
        }
        if (ql.tally) { tally_add(ql.tally, 3, nc); tally_add(ql.tally, 4, nc); }
        value[h] = (uint64_t)__popc(mask);
        rs[h] = (RS_MULTI << RS_MODE_SHIFT) | (uint64_t)sp | ((uint64_t)(rem + (LONG ? far[h] : 0)) << 32) | ((uint64_t)mask << 48);
      }
      if (qv[h] < n && !listed[h]) {
        counts[qv[h]] = value[h];
        if (ranges) { ranges[2 * qv[h]] = rs[h]; ranges[2 * qv[h] + 1] = 0; }
        if (status) status[qv[h]] = Q_OK;
      }
      const uint64_t lm = __ballot(listed[h]);
      if (lm) {
        unsigned int slot0 = 0;
        if (lane == 0) slot0 = atomicAdd(&s_count, (unsigned int)__popcll(lm));
        slot0 = __shfl(slot0, 0, 64);
        if (listed[h]) ql.q[region + slot0 + (uint64_t)__popcll(lm & lane_lt)] = (uint32_t)qv[h];
      }
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) ql.count[blockIdx.x] = s_count;
}

}  // namespace awry
