// edit_kernels.hip.h -- locate within k edits: a bit-vector edit-distance scan of text windows, and the glue that turns the
// located pieces of a query into those windows.
// Included by kernels.hip.h after its own kernels (it uses localise, backstep_scalar, symbol_at, ByteStream).
//
// No counterpart in the reference.  The definition, as include/awry_hip.h states it: T = the text without '$', n symbols;
//     D(s) = min over e in [s, n] of edit_distance(q, T[s..e))          (unit costs; D(-1) = D(n) = +inf)
//     s is a hit with distance D(s)  iff  D(s) <= k  and  D(s-1) >= D(s)  and  D(s+1) >= D(s)
// Pigeonhole: an alignment with <= k edits leaves one of the k + 1 pieces of q intact, so every s with D(s) <= k lies within k
// of a diagonal g - b_t (g: an occurrence of piece t, b_t: where the piece begins in q).  The diagonals of a query are sorted,
// neighbours at most 2k + 1 apart merged, and the run d_lo .. d_hi owns the starts [d_lo - k, d_hi + k]: owned ranges are
// disjoint.  edit_scan_kernel decides the hit rule for the owned starts of one window per lane.
//
// The scan runs RIGHT TO LEFT over T[max(lo - 1, 0) .. min(hi + L + k + 3, n)) with the REVERSED query, so that the score of
// a column is D at a START position (Myers 1999, the search recurrence: row 0 is free, the horizontal delta entering word 0
// is 0; blocks of 64 rows chained by their horizontal deltas as in Myers' block algorithm / Hyyro 2003).  Neighbouring D
// differ by at most 1 and a best alignment from s ends by s + L + D(s), so D is exact on [lo - 1, hi + 1] wherever it is
// <= k + 1, and a value the cut makes inexact is > k + 1 both truly and as computed.
#pragma once

namespace awry {

constexpr int EDIT_MAX_K = 8;      // AWRY_MAX_EDITS
constexpr int EDIT_MAX_LEN = 256;  // AWRY_EDIT_MAX_LEN
constexpr int EDIT_MAX_W = EDIT_MAX_LEN / 64;
constexpr uint8_t Q_CANDIDATE_CAP = 7;  // AWRY_Q_CANDIDATE_CAP: the pieces of the query occur more often than max_candidates

AWRY_HD constexpr int edit_symbols(int alphabet) { return alphabet == NUCLEOTIDE ? 5 : 21; }  // non-sentinel symbol indices 1 ..

// masks[(slot * S + s - 1) * W + w], bit j: letter L - 1 - (64 w + j) of the slot's query has symbol index s (the reversed
// query; bits at and above L are 0).  One lane per word.  slot_query == nullptr: slot i holds query i; else query slot_query[i].
template <int A>
__global__ __launch_bounds__(256) void edit_masks_kernel(const uint8_t* __restrict__ ascii, const uint64_t* __restrict__ off,
                                                         const uint32_t* __restrict__ slot_query, uint64_t nslots, int W, uint64_t* __restrict__ masks) {
  __shared__ uint8_t lut[256];
  lut[threadIdx.x] = (uint8_t)(threadIdx.x >= 128 ? 0xFF : index_of_ascii(A, (uint8_t)threadIdx.x));
  __syncthreads();
  constexpr uint64_t S = edit_symbols(A);
  const uint64_t per = S * (uint64_t)W, items = nslots * per, stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t it = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; it < items; it += stride) {
    const uint64_t slot = it / per, rem = it - slot * per;
    const uint32_t s = (uint32_t)(rem / (uint64_t)W) + 1u, w = (uint32_t)(rem % (uint64_t)W);
    const uint64_t q = slot_query ? slot_query[slot] : slot;
    const uint64_t b = off[q], e = off[q + 1];
    const uint64_t L = e > b && e - b <= 64ull * (uint64_t)W ? e - b : 0;  // (a query the scan does not take: no letters)
    ByteStream bytes(ascii);
    uint64_t m = 0;
    for (uint64_t j = 0; j < 64; j++) {
      const uint64_t i = 64ull * w + j;
      if (i < L) m |= (uint64_t)(lut[bytes[e - 1 - i]] == s) << j;
    }
    masks[it] = m;
  }
}

// One window per lane: the hits of query win_query[w] among the starts [win_first[w], win_first[w] + win_count[w]), cut to
// [0, n).  FILL = 0: n_hits[w].  FILL = 1: the hits in ascending position at gpos / edits [hit_off[w], hit_off[w + 1]) (the
// scan meets them in descending order and fills from the end; a slot below hit_off[w] is never written).
// W words of 64 rows per column, in registers (every index into pv / mv / eq is a constant after unrolling); the pattern
// masks of the column's symbol come from HBM / L2 (edit_masks_kernel wrote them; the windows of a query are neighbours in the
// list).  The text is read 8 symbols per load.  A hit needs the scores of three consecutive columns: two are kept back.
// A query the launch does not take -- empty, longer than 64 W, not longer than k -- has no hits.
// tally (nullable): [0] += text columns scanned, [1] += windows scanned.
template <int A, int W, bool FILL>
__global__ __launch_bounds__(256) void edit_scan_kernel(const uint8_t* __restrict__ text8, uint64_t n_text, const uint64_t* __restrict__ off,
                                                        const uint32_t* __restrict__ win_query, const uint64_t* __restrict__ win_first,
                                                        const uint32_t* __restrict__ win_count, uint64_t m, int k, const uint64_t* __restrict__ masks,
                                                        int masks_per_window, uint64_t* __restrict__ n_hits, const uint64_t* __restrict__ hit_off,
                                                        uint64_t* __restrict__ gpos, uint8_t* __restrict__ edits, unsigned long long* __restrict__ tally) {
  constexpr uint32_t S = edit_symbols(A);
  constexpr uint32_t INF = 0xFFFFu;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  const uint64_t* __restrict__ text = reinterpret_cast<const uint64_t*>(text8);
  unsigned long long t_cols = 0, t_wins = 0;
  for (uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; w < m; w += stride) {
    const uint64_t q = win_query[w];
    const uint64_t qb = off[q], qe = off[q + 1];
    const uint64_t L = qe > qb ? qe - qb : 0;
    const uint64_t first = win_first[w], cnt = win_count[w];
    uint64_t found = 0;
    if (L >= 1 && L <= 64ull * W && (uint64_t)k < L && cnt && first < n_text) {
      const uint64_t end = first + cnt < n_text ? first + cnt : n_text;  // owned starts [first, end)
      const uint64_t a = first ? first - 1 : 0;
      const uint64_t b = end - 1 + L + (uint64_t)k + 3 < n_text ? end - 1 + L + (uint64_t)k + 3 : n_text;  // scanned T[a, b)
      const uint64_t* __restrict__ pe = masks + (masks_per_window ? w : q) * (uint64_t)(S * W);
      const uint32_t lastw = (uint32_t)((L - 1) >> 6), lastbit = (uint32_t)((L - 1) & 63);
      uint64_t pv[W], mv[W];
#pragma unroll
      for (int i = 0; i < W; i++) { pv[i] = ~0ull; mv[i] = 0; }
      uint32_t score = (uint32_t)L, s1 = INF, s2 = INF;  // s1, s2: the scores one and two columns to the right (D(n) = +inf)
      const uint64_t out_lo = FILL ? hit_off[w] : 0;
      uint64_t out = FILL ? hit_off[w + 1] : 0;
      uint64_t word = 0, word_at = ~0ull;
      for (uint64_t j = b; j-- > a;) {
        if ((j >> 3) != word_at) { word_at = j >> 3; word = text[word_at]; }
        const uint32_t c = (uint32_t)(word >> (8 * (j & 7))) & 0xFFu;
        const bool letter = c - 1u < S;
        uint64_t eq[W];
#pragma unroll
        for (int i = 0; i < W; i++) eq[i] = letter ? pe[(c - 1u) * W + i] : 0ull;
        uint64_t hp = 0, hn = 0;  // the horizontal delta entering the word: +1 / -1 (row 0 is free: 0 into word 0)
#pragma unroll
        for (int i = 0; i < W; i++) {
          const uint64_t xv = eq[i] | mv[i];
          const uint64_t e2 = eq[i] | hn;
          const uint64_t xh = (((e2 & pv[i]) + pv[i]) ^ pv[i]) | e2;
          uint64_t ph = mv[i] | ~(xh | pv[i]);
          uint64_t mh = pv[i] & xh;
          if ((uint32_t)i == lastw) score += (uint32_t)((ph >> lastbit) & 1ull) - (uint32_t)((mh >> lastbit) & 1ull);
          const uint64_t hp2 = ph >> 63, hn2 = mh >> 63;
          ph = (ph << 1) | hp;
          mh = (mh << 1) | hn;
          pv[i] = mh | ~(xv | ph);
          mv[i] = ph & xv;
          hp = hp2;
          hn = hn2;
        }
        // score = D(j); decide the start j + 1 (>= first by the choice of a)
        if (j + 1 < end && s1 <= (uint32_t)k && s2 >= s1 && score >= s1) {
          found++;
          if (FILL && out > out_lo) { out--; gpos[out] = j + 1; edits[out] = (uint8_t)s1; }
        }
        s2 = s1;
        s1 = score;
      }
      if (a == first && s1 <= (uint32_t)k && s2 >= s1) {  // first == 0: the start 0, whose left neighbour is D(-1) = +inf
        found++;
        if (FILL && out > out_lo) { out--; gpos[out] = a; edits[out] = (uint8_t)s1; }
      }
      t_cols += b - a;
      t_wins++;
    }
    if (!FILL) n_hits[w] = found;
  }
  if (tally) {
    if (t_cols) atomicAdd(&tally[0], t_cols);
    if (t_wins) atomicAdd(&tally[1], t_wins);
  }
}

// ---- glue: pieces -> candidates -> diagonals -> windows ---------------------------------------------------------------

// Query q's pieces are the counts / statuses [q (k + 1), (q + 1)(k + 1)).  status[q] = the first non-zero piece status (a
// rejected query), else Q_CANDIDATE_CAP when the piece counts sum to more than max_candidates, else Q_OK; the piece counts of
// every query that is not Q_OK are zeroed, so that it has no candidates.
__global__ __launch_bounds__(256) void edit_cap_kernel(uint64_t* __restrict__ piece_counts, const uint8_t* __restrict__ piece_status, uint64_t n, int k,
                                                       uint64_t max_candidates, uint8_t* __restrict__ status) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x, w = (uint64_t)k + 1;
  for (uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; q < n; q += stride) {
    uint8_t st = Q_OK;
    uint64_t c = 0;
    for (uint64_t t = 0; t < w; t++) {
      if (st == Q_OK) st = piece_status[q * w + t];
      c += piece_counts[q * w + t];
    }
    if (st == Q_OK && c > max_candidates) st = Q_CANDIDATE_CAP;
    if (st != Q_OK)
      for (uint64_t t = 0; t < w; t++) piece_counts[q * w + t] = 0;
    status[q] = st;
  }
}

// out[i] = in[i * step] for i in [0, n): the candidate offsets of the queries out of the scanned piece offsets
__global__ __launch_bounds__(256) void edit_every_nth_kernel(const uint64_t* __restrict__ in, uint64_t n, uint64_t step, uint64_t* __restrict__ out) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) out[i] = in[i * step];
}

// largest i in [0, n) with off[i] <= h (off has n + 1 entries, off[0] <= h < off[n]): the owner of item h, empty owners skipped
__device__ __forceinline__ uint64_t edit_owner(const uint64_t* __restrict__ off, uint64_t n, uint64_t h) {
  uint64_t lo = 0, hi = n;
  while (hi - lo > 1) { const uint64_t mid = (lo + hi) >> 1; if (off[mid] <= h) lo = mid; else hi = mid; }
  return lo;
}

// located hit h of piece p = q (k + 1) + t -> the diagonal it lies on, as a key that sorts: position - piece begin + L (a
// read hanging over the text's start has a negative diagonal; the piece begins before L).  Piece t of a query of L letters is
// q[floor(t L / (k + 1)), floor((t + 1) L / (k + 1))).
__global__ __launch_bounds__(256) void edit_diagonals_kernel(const uint64_t* __restrict__ gpos, const uint64_t* __restrict__ piece_hit_off, uint64_t npieces,
                                                             uint64_t total, const uint64_t* __restrict__ off, int k, uint64_t* __restrict__ keys) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x, w = (uint64_t)k + 1;
  for (uint64_t h = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; h < total; h += stride) {
    const uint64_t p = edit_owner(piece_hit_off, npieces, h), q = p / w, t = p - q * w;
    const uint64_t L = off[q + 1] - off[q];
    keys[h] = gpos[h] + L - t * L / w;
  }
}

// a run of a query's sorted diagonals begins where the query's candidates begin or the gap to the left exceeds 2k + 1
// (duplicates and neighbours merge)
__device__ __forceinline__ bool edit_run_begins(const uint64_t* __restrict__ keys, uint64_t seg_begin, uint64_t j, int k) {
  return j == seg_begin || keys[j] - keys[j - 1] > 2ull * (uint64_t)k + 1;
}
__global__ __launch_bounds__(256) void edit_run_heads_kernel(const uint64_t* __restrict__ keys, const uint64_t* __restrict__ cand_off, uint64_t n,
                                                             uint64_t total, int k, uint64_t* __restrict__ heads) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < total; j += stride)
    heads[j] = edit_run_begins(keys, cand_off[edit_owner(cand_off, n, j)], j, k) ? 1 : 0;
}
// head_off = the exclusive scan of heads (total + 1 entries): run x = head_off[j + 1] - 1 holds diagonal j.  The first
// diagonal of a run writes the run's query and lowest key, the last one its highest key.
__global__ __launch_bounds__(256) void edit_run_ends_kernel(const uint64_t* __restrict__ keys, const uint64_t* __restrict__ cand_off, uint64_t n,
                                                            uint64_t total, int k, const uint64_t* __restrict__ head_off, uint32_t* __restrict__ win_query,
                                                            uint64_t* __restrict__ run_lo, uint64_t* __restrict__ run_hi) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < total; j += stride) {
    const uint64_t q = edit_owner(cand_off, n, j), x = head_off[j + 1] - 1;
    if (edit_run_begins(keys, cand_off[q], j, k)) { win_query[x] = (uint32_t)q; run_lo[x] = keys[j]; }
    if (j + 1 == cand_off[q + 1] || keys[j + 1] - keys[j] > 2ull * (uint64_t)k + 1) run_hi[x] = keys[j];
  }
}
// run (lo, hi) of keys -> the starts it owns: [lo - L - k, hi - L + k] cut to [0, n)
__global__ __launch_bounds__(256) void edit_windows_kernel(const uint32_t* __restrict__ win_query, const uint64_t* __restrict__ run_lo,
                                                           const uint64_t* __restrict__ run_hi, uint64_t m, const uint64_t* __restrict__ off, int k,
                                                           uint64_t n_text, uint64_t* __restrict__ win_first, uint32_t* __restrict__ win_count) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t x = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; x < m; x += stride) {
    const uint64_t q = win_query[x];
    const long long L = (long long)(off[q + 1] - off[q]);
    long long lo = (long long)run_lo[x] - L - k, hi = (long long)run_hi[x] - L + k;
    if (lo < 0) lo = 0;
    if (hi > (long long)n_text - 1) hi = (long long)n_text - 1;
    win_first[x] = (uint64_t)lo;
    win_count[x] = hi >= lo ? (uint32_t)(hi - lo + 1) : 0u;
  }
}
// hit offsets of the queries out of those of the windows: query i's first window is head_off[cand_off[i]] (every query's first
// diagonal begins a run), for i in [0, n]
__global__ __launch_bounds__(256) void edit_query_hit_off_kernel(const uint64_t* __restrict__ cand_off, const uint64_t* __restrict__ head_off,
                                                                 const uint64_t* __restrict__ win_hit_off, uint64_t n, uint64_t* __restrict__ out) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= n; i += stride) out[i] = win_hit_off[head_off[cand_off[i]]];
}

__global__ __launch_bounds__(256) void edit_localise_kernel(DevIndex ix, uint64_t total, const uint64_t* __restrict__ gpos, uint64_t* __restrict__ pos) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t h = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; h < total; h += stride) localise(ix, gpos[h], pos + 2 * h);
}

// The text as symbol indices without the dense SA: one LF chain per file SA sample, as densify_sa_kernel walks -- the row
// with SA = v holds BWT = T[v - 1] ('$' = T[bwt_len - 1] for v = 0) -- until the next sampled row, where another chain begins.
// 32-bit rows.
template <int A>
__global__ __launch_bounds__(256) void text8_chains_kernel(DevIndex ix, uint64_t nsamples, uint8_t* __restrict__ text8) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  const uint32_t fr = ix.sa_ratio;
  for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < nsamples; j += stride) {
    uint32_t row = (uint32_t)(j * fr);
    uint32_t v = (uint32_t)sa_sample(ix, j);
    for (;;) {
      text8[v ? (uint64_t)v - 1 : ix.bwt_len - 1] = (uint8_t)symbol_at<A>(ix, row);
      row = (uint32_t)backstep_scalar<A>(ix, row);
      if (row % fr == 0u) break;
      v--;
    }
  }
}

}  // namespace awry
