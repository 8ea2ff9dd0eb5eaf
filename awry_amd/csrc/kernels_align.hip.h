// kernels_align.hip.h -- align the hits of locate within k edits: the text span and one canonical CIGAR per hit, by a banded
// table with a traceback, one hit per lane.
// Included by kernels.hip.h after edit_kernels.hip.h (it uses edit_symbols, edit_owner, ByteStream, index_of_ascii).
//
// No counterpart in the reference.  The definition, as include/awry_hip.h states it, for a hit (q, s, d), d = D(s):
//     C[i][j] = edit_distance(q[0..i), T[s..s+j))       0 <= i <= L, 0 <= j <= J = min(L + d, n - s)
//     text_len = the smallest j with C[L][j] == d
//     traceback from (L, text_len): the diagonal first ('=' / 'X'), then 'I' (i--), then 'D' (j--)
// The kernel keeps only the band |i - j| <= d: a cell whose true value is <= d has its whole optimal path inside the band, so
// a banded value <= d is exact, and every equality the traceback tests involves such a value on one side.  The band of row i
// is indexed by the diagonal b = j - i + H, H = the launch's half-width (2, 4, 6 or 8, >= d): cells with |b - H| > d, j < 0 or
// j > J are +infinity.  Cell (i, b) has (i-1, b) on its diagonal, (i-1, b+1) above it and (i, b-1) to its left, so a row is
// updated in place in ascending b.
#pragma once

namespace awry {

constexpr int ALIGN_MAX_OPS = 2 * EDIT_MAX_K + 1;  // AWRY_ALIGN_MAX_OPS: d operations other than '=' separate at most d + 1 runs of '='
constexpr uint32_t ALIGN_INF = 0xFFFFu;

// the direction word of one row: 2 bits per band cell, cell b at bits [2b, 2b + 2): 0 '=', 1 'X', 2 'I', 3 'D'
template <int H>
struct AlignTrace {
  using word = std::conditional_t<(H <= 7), uint32_t, uint64_t>;  // 2 (2H + 1) bits: 10, 18, 26, 34
};

AWRY_HD constexpr uint32_t align_bam_op(uint32_t dir) { return dir == 0 ? 7u : dir == 1 ? 8u : dir == 2 ? 1u : 2u; }  // BAM: = 7, X 8, I 1, D 2

// One hit per lane, grid-stride: hit h is (query hit_query[h], start hit_gpos[h], distance hit_edits[h]).  Writes text_len[h],
// n_ops[h] and the runs ops[h * ALIGN_MAX_OPS .. + n_ops[h]) (len << 4 | BAM op), in query order.  A triple that is no
// alignment at that distance -- the minimum of row L inside the band of half-width hit_edits[h] differs from hit_edits[h], the
// start is >= n_text, the distance exceeds k, or the query is one the scan does not take (empty, longer than max_rows, not
// longer than k) -- gets n_ops = 0 and text_len = 0.
// The band (c[]) and the 2H + 1 text symbols under it (tw[], a window that slides by one per row) live in registers: every
// index is a constant after unrolling.  The text is read 8 symbols per load; the lanes of a wave mostly share the query.
// Row i's direction word goes to trace[(i - 1) * lanes_in_grid + lane], so that a wave's stores are contiguous; the traceback
// reads the lane's own words backwards.  trace holds max_rows * lanes_in_grid words.  The traceback meets the runs last to
// first: it writes them from the end of the hit's ops slot and moves them down at the end.
// tally (nullable): [0] += hits aligned, [1] += table cells computed (the cells of rows 0..L inside the band and the table).
template <int A, int H>
__global__ __launch_bounds__(256) void edit_align_kernel(const uint8_t* __restrict__ text8, uint64_t n_text, const uint8_t* __restrict__ ascii,
                                                         const uint64_t* __restrict__ off, const uint32_t* __restrict__ hit_query,
                                                         const uint64_t* __restrict__ hit_gpos, const uint8_t* __restrict__ hit_edits, uint64_t m, int k,
                                                         uint32_t max_rows, typename AlignTrace<H>::word* trace, uint32_t* __restrict__ text_len,
                                                         uint8_t* __restrict__ n_ops, uint32_t* ops, unsigned long long* __restrict__ tally) {
  using TW = typename AlignTrace<H>::word;
  constexpr int NB = 2 * H + 1;
  constexpr uint32_t S = edit_symbols(A);
  __shared__ uint8_t lut[256];
  lut[threadIdx.x] = (uint8_t)(threadIdx.x >= 128 ? 0xFF : index_of_ascii(A, (uint8_t)threadIdx.x));
  __syncthreads();
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x, lane = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t* __restrict__ text = reinterpret_cast<const uint64_t*>(text8);
  unsigned long long t_hits = 0, t_cells = 0;
  for (uint64_t h = lane; h < m; h += stride) {
    const uint64_t q = hit_query[h];
    const uint64_t qb = off[q], qe = off[q + 1];
    const uint64_t L64 = qe > qb ? qe - qb : 0;
    const uint64_t s = hit_gpos[h];
    const uint32_t d = hit_edits[h];
    uint32_t tl = 0, nops = 0;
    if (L64 >= 1 && L64 <= (uint64_t)max_rows && d <= (uint32_t)k && (uint64_t)k < L64 && k <= H && s < n_text) {
      const uint32_t L = (uint32_t)L64;
      const int J = (int)(n_text - s < (uint64_t)(L + d) ? n_text - s : (uint64_t)(L + d));
      uint64_t word = 0, word_at = ~0ull;
      auto symbol = [&](uint64_t p) -> uint32_t {  // T[p], 0 past the text's end
        if (p >= n_text) return 0u;
        if ((p >> 3) != word_at) { word_at = p >> 3; word = text[word_at]; }
        return (uint32_t)(word >> (8 * (p & 7))) & 0xFFu;
      };
      uint32_t c[NB], tw[NB];  // c[b] = C[i][i + b - H]; tw[b] = T[s + i + b - H - 1], the symbol cell b of row i compares
#pragma unroll
      for (int b = 0; b < NB; b++) {
        const int j = b - H;
        c[b] = j >= 0 && j <= (int)d && j <= J ? (uint32_t)j : ALIGN_INF;  // row 0
        tw[b] = j >= 0 ? symbol(s + (uint64_t)j) : 0u;                       // row 1
      }
      ByteStream qbytes(ascii);
      for (uint32_t i = 1; i <= L; i++) {
        if (i > 1) {
#pragma unroll
          for (int b = 0; b + 1 < NB; b++) tw[b] = tw[b + 1];
          tw[NB - 1] = symbol(s + (uint64_t)i + (uint64_t)(H - 1));
        }
        const uint32_t qs = lut[qbytes[qb + i - 1]];
        TW dirs = 0;
        uint32_t left = ALIGN_INF;
#pragma unroll
        for (int b = 0; b < NB; b++) {
          const int j = (int)i + b - H;
          const uint32_t neq = tw[b] == qs && tw[b] - 1u < S ? 0u : 1u;
          const uint32_t dg = c[b] + neq, up = (b + 1 < NB ? c[b + 1] : ALIGN_INF) + 1u, lf = left + 1u;
          uint32_t v = dg < up ? dg : up;
          v = v < lf ? v : lf;
          uint32_t dir = dg == v ? neq : (up == v ? 2u : 3u);
          if (j == 0) { v = i; dir = 2u; }  // column 0: only 'I' leads back
          const int off_diag = b > H ? b - H : H - b;
          if (j < 0 || j > J || (uint32_t)off_diag > d) v = ALIGN_INF;
          c[b] = v;
          left = v;
          dirs |= (TW)dir << (2 * b);
        }
        trace[(uint64_t)(i - 1) * stride + lane] = dirs;
        if (tally) {
          const int lo = (int)i > (int)d ? (int)i - (int)d : 0, hi = (int)(i + d) < J ? (int)(i + d) : J;
          if (hi >= lo) t_cells += (unsigned long long)(hi - lo + 1);
        }
      }
      uint32_t mn = ALIGN_INF;
      int b = 0;
#pragma unroll
      for (int x = 0; x < NB; x++)
        if (c[x] < mn) { mn = c[x]; b = x; }  // the first minimum: the smallest end
      if (mn == d) {
        bool ok = true;
        uint32_t i = L, j = L + (uint32_t)b - (uint32_t)H, slot = ALIGN_MAX_OPS, run_op = 0, run_len = 0, row = 0;
        tl = j;
        uint32_t* my = ops + h * (uint64_t)ALIGN_MAX_OPS;
        TW dirs = 0;
        while (i | j) {
          uint32_t dir = 3u;  // row 0: only 'D' leads back
          if (i) {
            if (row != i) { row = i; dirs = trace[(uint64_t)(i - 1) * stride + lane]; }
            dir = (uint32_t)(dirs >> (2 * b)) & 3u;
          }
          const uint32_t op = align_bam_op(dir);
          if (op != run_op) {
            if (run_len) {
              if (slot == 0) { ok = false; break; }
              my[--slot] = run_len << 4 | run_op;
            }
            run_op = op;
            run_len = 0;
          }
          run_len++;
          if (dir <= 1u) { i--; j--; }
          else if (dir == 2u) { i--; b++; }
          else { j--; b--; }
          if ((uint32_t)b >= (uint32_t)NB || (int)j < 0) { ok = false; break; }  // (never on a consistent table)
        }
        if (ok && run_len) {
          if (slot == 0) ok = false;
          else my[--slot] = run_len << 4 | run_op;
        }
        if (ok) {
          nops = ALIGN_MAX_OPS - slot;
          if (slot)
            for (uint32_t x = 0; x < nops; x++) my[x] = my[slot + x];
          t_hits++;
        } else {
          tl = 0;
        }
      }
      if (tally) t_cells += (unsigned long long)((int)d < J ? (int)d : J) + 1ull;  // row 0
    }
    text_len[h] = tl;
    n_ops[h] = (uint8_t)nops;
  }
  if (tally) {
    if (t_hits) atomicAdd(&tally[0], t_hits);
    if (t_cells) atomicAdd(&tally[1], t_cells);
  }
}

// hit h of a chunk lies in window edit_owner(win_hit_off, m, h): its query
__global__ __launch_bounds__(256) void align_hit_query_kernel(const uint64_t* __restrict__ win_hit_off, const uint32_t* __restrict__ win_query, uint64_t m,
                                                              uint64_t nhits, uint32_t* __restrict__ hit_query) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t h = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; h < nhits; h += stride) hit_query[h] = win_query[edit_owner(win_hit_off, m, h)];
}

// fixed stride -> CSR: the run counts as scan input, then the runs of hit h to cigar[cigar_off[h] ..)
__global__ __launch_bounds__(256) void align_counts_kernel(const uint8_t* __restrict__ n_ops, uint64_t m, uint64_t* __restrict__ counts) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t h = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; h < m; h += stride) counts[h] = n_ops[h];
}
__global__ __launch_bounds__(256) void align_compact_kernel(const uint32_t* __restrict__ ops, const uint8_t* __restrict__ n_ops,
                                                            const uint64_t* __restrict__ cigar_off, uint64_t m, uint32_t* __restrict__ cigar) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t h = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; h < m; h += stride) {
    const uint32_t cnt = n_ops[h] <= ALIGN_MAX_OPS ? n_ops[h] : 0u;
    const uint64_t at = cigar_off[h];
    for (uint32_t x = 0; x < cnt; x++) cigar[at + x] = ops[h * (uint64_t)ALIGN_MAX_OPS + x];
  }
}

}  // namespace awry
