// kernels_reads.hip.h -- packed reads of any length: the single-kernel schedule, the probe pass and the listed / pooled second passes.
// A part of kernels.hip.h (one header, cut by kernel family): included there, in order, and not on its own.
#pragma once

namespace awry {

// Packed reads of any length (W = ceil(L/32) words per query, letter j in word j/32, bits 2(j%32)): the quad design
// of the k-mer kernels, the current word re-read every 32 letters, the final range handed on for locate.
//
// VERIFY adds seed-and-verify, an MI355X-first shortcut the 288 GB of HBM pay for (dense SA + 4-bit text resident):
// once the range has shrunk to <= 8 rows, the remaining i symbols are not matched by i dependent LF steps (i random
// lines) but by comparing them with the text in front of each candidate suffix: 1 SA read + the i/2 contiguous bytes
// of text per candidate.  The rows that survive are exactly the rows whose suffixes extend to the whole query, in
// the same relative order as the final range (the suffixes share everything after the seed part), so counts and
// locations are unchanged; the locate pass receives the verified candidates instead of a row range (RS_* words).
// LIST: the quads of block b work through the reads block b of count_nt2_reads_probe_kernel left undecided
// (sv.q / sv.count, same grid) instead of all n reads.
// RAGGED: read q has lens[q] letters (1 <= lens[q] <= L); L only sets the stride of W words per read.
// (the kernel's body as a block-level function -- LIST: the block's quads work through list_q[0 .. n) -- so that
//  lcx_quad_reads_kernel can run it over what its lanes left undecided; allow_lcx = false there: those reads take LF steps)
template <bool USE_SEED, bool VERIFY, bool LIST, bool RAGGED>
__device__ __forceinline__ void reads_body(const DevIndex& ix, const uint64_t* __restrict__ queries, uint64_t n, int L,
                                           uint64_t* __restrict__ counts, uint64_t* __restrict__ range_start,
                                           const uint32_t* __restrict__ list_q, const uint32_t* __restrict__ lens, bool allow_lcx,
                                           uint64_t r_start = ~0ull, uint64_t r_stride = 64) {
  const int l = threadIdx.x & 3;
  const uint64_t nquads = ((uint64_t)gridDim.x * blockDim.x) >> 2;
  uint64_t r = r_start == ~0ull ? threadIdx.x >> 2 : r_start;  // LIST: position in the list (a block's own: its 64 quads)
  uint64_t q = LIST ? (r < n ? list_q[r] : 0) : ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 2;
  const uint64_t* __restrict__ blocks = ix.blocks;
  const SeedEntry* __restrict__ seed = ix.seed;
  const uint32_t* __restrict__ dense = ix.dense_sa;
  const uint32_t* __restrict__ text4 = ix.text4;
  const int k = USE_SEED ? ix.seed_k : 1, W = (L + 31) / 32;
  const int verify_after = (int)ix.verify_after;
  // left-context index (layout.h): a seed range of 2+ rows is narrowed by a search over its bucket's keys -- the 32 letters
  // left of the seed window in log16(rows) lines -- instead of one LF step per letter; what is left is compared with the text
  const bool lcx = USE_SEED && VERIFY && ix.lcx_key != nullptr && allow_lcx;
  const uint32_t cA = (uint32_t)ix.prefix_sums[1], cC = (uint32_t)ix.prefix_sums[2], cG = (uint32_t)ix.prefix_sums[3],
                 cN = (uint32_t)ix.prefix_sums[4], cT = (uint32_t)ix.prefix_sums[5], cEnd = (uint32_t)ix.prefix_sums[6];
  bool have = LIST ? r < n : q < n, fresh = true;
  uint64_t w = 0;
  uint32_t sp = 1, ep = 0;
  int i = 0, steps_done = 0;
  // quad-uniform state: mode 0 = LF steps, 1 = text position of candidate vj, 2 = compare text chunk vc;
  // left-context index: 3 = number of incomplete entries of the bucket, 4 = search its keys
  int mode = 0, vj = 0, vc = 0;
  uint32_t vmask = 0, vp = 0;
  bool pos_hit = false;  // position seed whose window is the whole read
  bool cand_lcx = false;  // modes 1 / 2: candidates sp..ep are entries of the left-context index, not rows
  bool tail_pass = false; // modes 1 / 2: the candidates are the bucket's incomplete entries (after the key search)
  LcxQ lq{0, 0, 0, 0, -1};
  uint64_t qlo = 0, qhi = 0;
  uint32_t b_sp = 0, b_cnt = 0, b_inc = 0, key_hits = 0, key_lb = 0;
  while (__any(have)) {
    if (have) {
      const uint64_t* qw = queries + q * W;
      bool finished = false;
      uint64_t out_count = 0, out_rs = 0;
      const bool hole = LIST && q == 0xFFFFFFFFull;  // an empty slot of lcx_quad_reads_kernel's list: nothing to do
      if (hole) {
        finished = true;
      } else if (mode == 0) {
        if (fresh) {
          const int Lq = RAGGED ? (int)lens[q] : L;
          const bool seeded = USE_SEED && (!RAGGED || Lq >= k);  // a read shorter than the seed starts without the table
          const int first = seeded ? Lq - k : 0;  // letters first .. Lq-1 form the seed window (leftmost letter least significant)
          const int a = first >> 5, sh = 2 * (first & 31);
          uint64_t win = qw[a] >> sh;
          if (sh && a + 1 < W) win |= qw[a + 1] << (64 - sh);
          SeedEntry e{1u, 0u};
          uint32_t scnt = SEED_CNT_SAT;
          if (seeded) {
            e = seed[(win & ((1ull << (2 * k)) - 1))];
            scnt = seed_entry_range(e, sp, ep);
            i = first;
          }
          if (!seeded || scnt == SEED_CNT_SAT) {  // no table, or a count the entry cannot represent
            const uint32_t c = nt2_letter_at(qw, Lq - 1);  // SearchRange::new(last letter)
            sp = c == 0 ? cA : (c == 1 ? cC : (c == 2 ? cG : cT));
            ep = (c == 0 ? cC : (c == 1 ? cG : (c == 2 ? cN : cEnd))) - 1;
            i = Lq - 1;
          }
          steps_done = 0;
          w = i > 0 ? qw[(i - 1) >> 5] : 0;
          if (USE_SEED) seed_singleton_check(e, scnt, w, 2 * ((i - 1) & 31), i, sp, ep);
          if (seeded && ix.seed_pos && scnt == 1u && sp <= ep) {
            // position seed: e.sp is SA[row], the text position of the single candidate -- there is no row to step from
            if (i == 0) {  // the read is the seed window itself
              pos_hit = true;
              vp = seed_position(e, (int)ix.ctx_extra);
            } else if (VERIFY && i < 65536) {  // straight to the text, no SA read
              vp = seed_position(e, (int)ix.ctx_extra);
              sp = ep = 0u;  // one candidate, index 0
              vj = 0;
              vmask = 0;
              cand_lcx = tail_pass = false;
              if (vp >= (uint32_t)i) { mode = 2; vc = 0; }
              else { mode = 1; vj = 1; }  // too close to the text's beginning: no match (finishes below)
            } else {  // start again without the table
              const uint32_t c = nt2_letter_at(qw, Lq - 1);
              sp = c == 0 ? cA : (c == 1 ? cC : (c == 2 ? cG : cT));
              ep = (c == 0 ? cC : (c == 1 ? cG : (c == 2 ? cN : cEnd))) - 1;
              i = Lq - 1;
              w = i > 0 ? qw[(i - 1) >> 5] : 0;
            }
          } else if (lcx && seeded && scnt >= 2u && scnt != SEED_CNT_SAT && !(e.cnt & SEED_LCX_NONE) && i > 0 && i < 65536) {
            b_sp = sp;
            b_cnt = scnt;
            b_inc = 0;
            lcx_thresholds(lcx_read_ctx(qw, W, i), i < LCX_CTX ? i : LCX_CTX, &qlo, &qhi);
            if (e.cnt & SEED_LCX_TAIL) mode = 3;
            else { lcx_begin(lq, b_sp, b_cnt); mode = 4; }
          }
          fresh = false;
        } else {
          i--;
          const uint32_t c = (uint32_t)(w >> (2 * (i & 31))) & 3u;
          const uint32_t cl = c == 0 ? cA : (c == 1 ? cC : (c == 2 ? cG : cT));
          quad_step(blocks, cl, sp, ep, c, l);
          steps_done++;
          if ((i & 31) == 0 && i > 0) w = qw[(i - 1) >> 5];
        }
        if (pos_hit) {
          finished = true;
          pos_hit = false;
          out_count = 1;
          out_rs = (RS_SINGLE << RS_MODE_SHIFT) | (uint64_t)vp;
        } else if (mode != 0) {
          // a position seed went straight to the text / the bucket's keys are searched
        } else if (sp > ep || i == 0) {
          finished = true;
          out_count = sp > ep ? 0ull : (uint64_t)(ep - sp) + 1ull;
          out_rs = (RS_PLAIN << RS_MODE_SHIFT) | sp;
        } else if (VERIFY) {
          const uint32_t cnt = ep - sp + 1u;
          if (verify_now(cnt, i, steps_done, verify_after) && i < 65536) { mode = 1; vj = 0; vmask = 0; cand_lcx = tail_pass = false; }
        }
      } else if (mode == 1) {  // text position of candidate vj: row sp + vj, or entry sp + vj of the left-context index
        vp = cand_lcx ? (uint32_t)ix.lcx_rowpos[sp + (uint32_t)vj] : dense[sp + (uint32_t)vj];
        if (vp >= (uint32_t)i) { mode = 2; vc = 0; }
        else vj++;  // the suffix starts too close to the text's beginning to have i symbols in front
      } else if (mode == 2) {      // compare window chunk vc of candidate vj
        const uint64_t g = (uint64_t)vp - (uint64_t)i;
        const int wi = 4 * vc + l;
        const uint32_t bad = quad_sum(verify_part(text4, g, i, vc, l, wi < W ? qw[wi] : 0ull));
        if (bad) { vj++; mode = 1; }
        else if (128 * (vc + 1) < i) vc++;
        else { vmask |= 1u << vj; vj++; mode = 1; }
      } else if (mode == 3) {  // the key slot of the bucket's last row holds the number of incomplete entries
        b_inc = (uint32_t)ix.lcx_key[b_sp + b_cnt - 1u];
        // (they can only match a read with fewer than 32 letters left of its seed window; more of them than are worth
        //  checking one by one: LF steps after all)
        if (i < LCX_CTX && b_inc > (uint32_t)LCX_TAIL_MAX) mode = 0;
        else { lcx_begin(lq, b_sp, b_cnt - b_inc); mode = 4; }
      } else {  // mode 4
        lcx_quad_step(ix, lq, qlo, qhi, l);
        if (lq.t < 0) {
          key_lb = lq.a0;
          key_hits = lq.a1 - lq.a0;
          if (i <= LCX_CTX) {
            // the keys hold every letter the read has left: the run IS the answer, but for the bucket's incomplete entries
            if (b_inc && i < LCX_CTX) {  // (at most LCX_TAIL_MAX <= 32 of them: vmask has a bit each)
              sp = b_sp + (b_cnt - b_inc); ep = b_sp + b_cnt - 1u;
              cand_lcx = tail_pass = true;
              mode = 1; vj = 0; vmask = 0;
            } else if (!range_start || key_hits <= 8u) {
              finished = true;
              out_count = key_hits;
              out_rs = key_hits ? ((RS_LCX << RS_MODE_SHIFT) | (uint64_t)key_lb | ((uint64_t)i << 32) | ((uint64_t)((1u << key_hits) - 1u) << 48))
                                : ((RS_PLAIN << RS_MODE_SHIFT) | 1ull);
            } else mode = 0;  // the locate pass wants the rows of a larger range: LF steps from the seed range
          } else if (key_hits == 0u) {
            finished = true;
            out_rs = (RS_PLAIN << RS_MODE_SHIFT) | 1ull;
          } else if (key_hits <= 8u) {  // the entries that agree on 32 letters: the rest of each is compared with the text
            sp = key_lb; ep = key_lb + key_hits - 1u;
            cand_lcx = true; tail_pass = false;
            mode = 1; vj = 0; vmask = 0;
          } else mode = 0;  // too many candidates still (a young or exact repeat): LF steps from the seed range
          if (mode == 0) { sp = b_sp; ep = b_sp + b_cnt - 1u; }
        }
      }
      if (VERIFY && mode == 1 && vj > (int)(ep - sp)) {  // all candidates checked
        if (tail_pass) {  // the bucket's incomplete entries: they add to the run the keys selected
          const uint32_t th = (uint32_t)__popc(vmask);
          tail_pass = cand_lcx = false;
          if (!range_start || (th == 0u && key_hits <= 8u)) {
            finished = true;
            out_count = (uint64_t)key_hits + th;
            out_rs = key_hits ? ((RS_LCX << RS_MODE_SHIFT) | (uint64_t)key_lb | ((uint64_t)i << 32) | ((uint64_t)((1u << key_hits) - 1u) << 48))
                              : ((RS_PLAIN << RS_MODE_SHIFT) | 1ull);
          } else { mode = 0; sp = b_sp; ep = b_sp + b_cnt - 1u; }
        } else {
          finished = true;
          out_count = (uint64_t)__popc(vmask);
          if (ep == sp && vmask) out_rs = (RS_SINGLE << RS_MODE_SHIFT) | ((uint64_t)vp - (uint64_t)i);
          else out_rs = ((cand_lcx ? RS_LCX : RS_MULTI) << RS_MODE_SHIFT) | (uint64_t)sp | ((uint64_t)i << 32) | ((uint64_t)vmask << 48);
          cand_lcx = false;
        }
      }
      if (finished) {
        if (l == 0 && !hole) {
          counts[q] = out_count;
          if (range_start) range_start[q] = out_rs;
        }
        if (LIST) {
          r += r_stride;
          have = r < n;
          q = have ? list_q[r] : 0;
        } else {
          q += nquads;
          have = q < n;
        }
        fresh = true;
        mode = 0;
      }
    }
  }
}

template <bool USE_SEED, bool VERIFY, bool LIST = false, bool RAGGED = false>
__global__ __launch_bounds__(256) void count_nt2_reads_kernel(DevIndex ix, const uint64_t* __restrict__ queries, uint64_t n, int L,
                                                              uint64_t* __restrict__ counts, uint64_t* __restrict__ range_start,
                                                              Nt2Survivors sv = Nt2Survivors{}, const uint32_t* __restrict__ lens = nullptr) {
  if (LIST) reads_body<USE_SEED, VERIFY, LIST, RAGGED>(ix, queries, (uint64_t)sv.count[blockIdx.x], L, counts, range_start, sv.q + (uint64_t)blockIdx.x * sv.cap, lens, true);
  else reads_body<USE_SEED, VERIFY, LIST, RAGGED>(ix, queries, n, L, counts, range_start, nullptr, lens, true);
}
// one device-wide list of reads (sv.count[0] of them at sv.q[0 ..)), walked by all quads of the grid with LF steps: what
// lcx_quad_reads_kernel could not settle
template <bool RAGGED>
__global__ __launch_bounds__(256) void count_nt2_reads_pool_kernel(DevIndex ix, const uint64_t* __restrict__ queries, int L, uint64_t* __restrict__ counts,
                                                                   uint64_t* __restrict__ range_start, Nt2Survivors sv, const uint32_t* __restrict__ lens) {
  reads_body<true, true, true, RAGGED>(ix, queries, (uint64_t)sv.count[0], L, counts, range_start, sv.q, lens, false,
                                       ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 2, ((uint64_t)gridDim.x * blockDim.x) >> 2);
}

// Phase 1 of the two-phase schedule for reads (seed table + dense SA + 4-bit text resident, 3 <= L - k): one read per
// LANE.  The seed entry alone settles reads whose seed k-mer is absent or a singleton with the wrong BWT symbol; a
// singleton with the right symbol is one candidate, settled by SA[sp] and the L - k letters of text in front of it
// (queued in LDS so that full waves issue those loads, as in count_nt2_probe_kernel); the rest (2+ rows, saturated
// entries) goes to block-private lists that count_nt2_reads_kernel<.., LIST> works through with the quad machinery.
// Results are those of count_nt2_reads_kernel<true, true> (counts and RS_* range-start words).  RAGGED: read q has
// lens[q] letters; reads with fewer than 3 letters left of their seed window go to the lists unprobed.
template <bool RAGGED>
__global__ __launch_bounds__(256) void count_nt2_reads_probe_kernel(DevIndex ix, const uint64_t* __restrict__ queries, uint64_t n, int L,
                                                                    uint64_t* __restrict__ counts, uint64_t* __restrict__ range_start,
                                                                    Nt2Survivors sv, const uint32_t* __restrict__ lens) {
  constexpr int VQ = 192;
  __shared__ unsigned int s_count;
  __shared__ uint32_t s_vsp[4][VQ], s_vq[4][VQ];
  __shared__ uint8_t s_vn[4][VQ];
  __shared__ uint16_t s_vl[RAGGED ? 4 : 1][VQ];  // RAGGED: the read's length (<= 512 on this path)
  __shared__ uint64_t s_vw[4][3][VQ];  // the letters left of the seed window of a queued read (<= 96 of them: three words)
  if (threadIdx.x == 0) s_count = 0;
  if (blockIdx.x == 0 && threadIdx.x == 0 && sv.lf_count) *sv.lf_count = 0;
  __syncthreads();
  const int lane = threadIdx.x & 63, wv_id = threadIdx.x >> 6;
  const SeedEntry* __restrict__ seed = ix.seed;
  const int k = ix.seed_k, W = (L + 31) / 32;  // RAGGED: L is the longest read, W the stride
  const bool pos = ix.seed_pos != 0;           // singleton entries hold SA[row]: no SA read, and no row to step from
  const int min_i0 = pos ? 1 : 3;              // fewest letters left of the seed window worth (or, with pos, needing) the text
  const int cx = (int)ix.ctx_extra, clen = SEED_CTX_LEN + cx;  // letters in front of the occurrence a context entry holds
  const uint64_t kmask = (1ull << (2 * k)) - 1;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  const uint64_t lane_lt = (1ull << lane) - 1;
  const uint64_t region = (uint64_t)blockIdx.x * sv.cap;
  // a queued read is compared with the text a few hundred seed probes after its words were read: by then the random seed
  // lines have pushed them out of L2, so the words wait in LDS beside the queue entry instead of being fetched again
  const bool stash = L - k <= 96;
  int vcount = 0;
  auto settle = [&](uint64_t q, uint64_t count, uint64_t rs) {
    counts[q] = count;
    if (range_start) range_start[q] = rs;
  };
  auto drain = [&](int base, int cnt) {  // queue entries [base, base + cnt), cnt <= 128: two per lane
    uint32_t q[2], sp[2], nc[2], vp[2];
    bool on[2];
#pragma unroll
    for (int h = 0; h < 2; h++) {
      const int s = base + lane + 64 * h;
      on[h] = lane + 64 * h < cnt;
      q[h] = on[h] ? s_vq[wv_id][s] : 0;
      sp[h] = on[h] ? s_vsp[wv_id][s] : 0;
      nc[h] = on[h] ? s_vn[wv_id][s] : 0;
      vp[h] = on[h] ? ((pos && nc[h] == 1u) ? sp[h] : ix.dense_sa[sp[h]]) : 0;
    }
#pragma unroll
    for (int h = 0; h < 2; h++) {
      if (!on[h]) continue;
      const int i0 = (RAGGED ? (int)s_vl[RAGGED ? wv_id : 0][base + lane + 64 * h] : L) - k, nchunks = (i0 + 31) >> 5;
      const uint64_t* qw = queries + (uint64_t)q[h] * W;
      uint32_t mask = 0;
      uint64_t g1 = 0;
      for (uint32_t c2 = 0; c2 < nc[h]; c2++) {  // the rows of a range are neighbours in the dense SA: mostly one line
        const uint32_t p = c2 ? ix.dense_sa[sp[h] + c2] : vp[h];
        uint32_t bad = p >= (uint32_t)i0 ? 0u : 1u;  // else the suffix starts too close to the text's beginning
        const uint64_t g = (uint64_t)p - (uint64_t)i0;
        for (int c = 0; c < nchunks && !bad; c++)
          bad = verify_part(ix.text4, g, i0, c >> 2, c & 3, stash ? s_vw[wv_id][c][base + lane + 64 * h] : qw[c]);
        if (!bad) { mask |= 1u << c2; g1 = g; }
      }
      if (nc[h] == 1u && mask) settle(q[h], 1, (RS_SINGLE << RS_MODE_SHIFT) | g1);
      else settle(q[h], (uint64_t)__popc(mask), (RS_MULTI << RS_MODE_SHIFT) | (uint64_t)sp[h] | ((uint64_t)i0 << 32) | ((uint64_t)mask << 48));
    }
  };
  constexpr int NQ = 2;  // reads in flight per lane (3 and 4 measure the same)
  for (uint64_t wbase = (uint64_t)blockIdx.x * blockDim.x + (threadIdx.x & ~63u); wbase < n; wbase += NQ * stride) {
    uint64_t qv[NQ], win[NQ];
    uint64_t lw[NQ][3];
    uint32_t nc[NQ];
    bool probe[NQ];  // false: too short for the per-lane path (fewer than 3 letters left of the seed window)
    SeedEntry ev[NQ];
#pragma unroll
    for (int h = 0; h < NQ; h++) {
      qv[h] = wbase + lane + (uint64_t)h * stride;
      win[h] = 0;
      nc[h] = 0;
      probe[h] = false;
      if (qv[h] < n) {
        const int i0 = (RAGGED ? (int)lens[qv[h]] : L) - k;
        probe[h] = i0 >= min_i0;
        if (probe[h]) {
          const uint64_t* qw = queries + qv[h] * W;
          const int wa = i0 >> 5, wsh = 2 * (i0 & 31);            // seed window: letters i0 .. L-1
          const int na = (i0 - 1) >> 5, nsh = 2 * ((i0 - 1) & 31);  // the letter in front of it
          win[h] = qw[wa] >> wsh;
          if (wsh && wa + 1 < W) win[h] |= qw[wa + 1] << (64 - wsh);
          nc[h] = (uint32_t)(qw[na] >> nsh) & 3u;
          if (stash) {
#pragma unroll
            for (int c = 0; c < 3; c++) lw[h][c] = c < W ? qw[c] : 0;
          }
        }
      }
    }
#pragma unroll
    for (int h = 0; h < NQ; h++) {
      ev[h] = SeedEntry{1u, 0u};
      if (probe[h]) ev[h] = seed_probe(seed + (win[h] & kmask));
    }
#pragma unroll
    for (int h = 0; h < NQ; h++) {
      const bool valid = qv[h] < n;
      const SeedEntry e = ev[h];
      const uint32_t cnt = seed_cnt(e);
      bool survivor = false, queued = false;
      if (valid && !probe[h]) {
        survivor = true;
      } else if (valid) {
        if (cnt == 0u) settle(qv[h], 0, (RS_PLAIN << RS_MODE_SHIFT) | 1ull);
        else if (cnt == 1u && pos && seed_has_ctx(e)) {
          // the entry holds the letters in front of the one occurrence: a read with no more than that left of its
          // seed window is decided here; a longer one goes on to the text only if they agree
          const int i0 = (RAGGED ? (int)lens[qv[h]] : L) - k;
          const uint64_t* qw = queries + qv[h] * W;
          if (i0 <= clen) {
            const bool same = (qw[0] & ((1ull << (2 * i0)) - 1)) == (seed_full_ctx(e, cx) >> (2 * (clen - i0)));
            settle(qv[h], same ? 1 : 0,
                   same ? ((RS_SINGLE << RS_MODE_SHIFT) | (uint64_t)(seed_position(e, cx) - (uint32_t)i0)) : ((RS_PLAIN << RS_MODE_SHIFT) | 1ull));
          } else {
            const int f = i0 - clen, a = f >> 5, sh = 2 * (f & 31);
            uint64_t x = qw[a] >> sh;
            if (sh && a + 1 < W) x |= qw[a + 1] << (64 - sh);
            queued = (x & ((1ull << (2 * clen)) - 1)) == seed_full_ctx(e, cx);
            if (!queued) settle(qv[h], 0, (RS_PLAIN << RS_MODE_SHIFT) | 1ull);
          }
        } else if (cnt == 1u) {
          queued = seed_sym(e) == (int)(nc[h] == 3u ? 5u : nc[h] + 1u);
          if (!queued) settle(qv[h], 0, (RS_PLAIN << RS_MODE_SHIFT) | 1ull);  // BWT[sp] is not the next letter: absent
        } else if (cnt <= (uint32_t)VMULTI && (int)(3u * cnt) <= (RAGGED ? (int)lens[qv[h]] : L) - k) {
          queued = true;  // a handful of candidate rows: each is checked against the text here
        } else survivor = true;  // more rows, or a saturated entry
      }
      const uint64_t qm = __ballot(queued);
      if (qm) {
        if (queued) {
          const int s = vcount + (int)__popcll(qm & lane_lt);
          s_vsp[wv_id][s] = cnt == 1u && pos ? seed_position(e, cx) : e.sp;
          s_vq[wv_id][s] = (uint32_t)qv[h];
          s_vn[wv_id][s] = (uint8_t)cnt;
          if (RAGGED) s_vl[wv_id][s] = (uint16_t)lens[qv[h]];
          if (stash) {
#pragma unroll
            for (int c = 0; c < 3; c++) s_vw[wv_id][c][s] = lw[h][c];
          }
        }
        vcount += (int)__popcll(qm);
        __builtin_amdgcn_wave_barrier();
        if (vcount >= 128) {
          vcount -= 128;
          drain(vcount, 128);
          __builtin_amdgcn_wave_barrier();
        }
      }
      const uint64_t sm = __ballot(survivor);
      if (sm) {
        unsigned int slot0 = 0;
        if (lane == 0) slot0 = atomicAdd(&s_count, (unsigned int)__popcll(sm));
        slot0 = __shfl(slot0, 0, 64);
        if (survivor) {
          const uint64_t s = region + slot0 + (uint64_t)__popcll(sm & lane_lt);
          sv.q[s] = (uint32_t)qv[h];
          if (sv.range) {  // for lcx_quad_reads_kernel: the probed entry (~0: not probed) and the <= 32 letters left of the seed window
            sv.range[s] = probe[h] ? ((uint64_t)e.sp | ((uint64_t)(cnt | (e.cnt & (SEED_LCX_NONE | SEED_LCX_TAIL))) << 32)) : ~0ull;
            sv.w[s] = probe[h] ? lcx_read_ctx(queries + qv[h] * W, W, (RAGGED ? (int)lens[qv[h]] : L) - k) : 0ull;
          }
        }
      }
    }
  }
  if (vcount > 0) drain(0, vcount);
  __syncthreads();
  if (threadIdx.x == 0) sv.count[blockIdx.x] = s_count;
}

}  // namespace awry
