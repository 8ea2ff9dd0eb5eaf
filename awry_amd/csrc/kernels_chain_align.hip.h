// kernels_chain_align.hip.h -- align chains: the members of a chain as diagonal pieces, banded tables for the query before the
// first piece (left extension), between pieces (gaps) and after the last (right extension), one CIGAR over the whole read.
// Included by kernels.hip.h after kernels_chain.hip.h (it uses Seed, ByteStream, edit_symbols, index_of_ascii, align_bam_op).
//
// No counterpart in the reference.  The definition is the one include/awry_hip.h states ("align chains"); in short, for a segment
// that aligns x (a query letters) to a prefix of y (text letters, J columns), with skew m and band parameter W:
//     band: lo <= j - i <= hi, lo = min(0, m) - W, hi = max(0, m) + W; cells outside it, or with j > J, are +infinity
//     gap:        m = b - a, J = b, the alignment ends at (a, b)
//     extension:  m = min(0, avail - a), J = min(a + W, avail), it ends at the smallest j that minimises row a
//     traceback:  the diagonal first ('=' / 'X'), then 'I' (i--), then 'D' (j--)
// The band of row i is indexed by b = j - i - lo, 0 <= b < NB = hi - lo + 1 <= NBMAX, the instantiation's width: as in
// edit_align_kernel, cell (i, b) has (i-1, b) on its diagonal, (i-1, b+1) above it and (i, b-1) to its left, a row is updated in
// place in ascending b, and every index into the band is a constant after unrolling.  Cells at b >= NB are +infinity.
//
// Chains are classified by their widest segment (chain_align_classify_kernel): NB <= 9, <= 17, <= 33.  Each class is one
// instantiation over the class's list of chain indices, so a lane pays for the cells of its class only.  Chains that are not
// aligned (AWRY_ALN_BAD_CHAIN, AWRY_ALN_SKEW) get their record from the classify kernel and enter no list.
//
// CLIP = true is the clipped mode of the same kernels (include/awry_hip.h, "soft-clip read ends"): pieces and gaps as above, the two
// extensions scored and local.  The row update minimises a signed cost with per-segment weights (match, mismatch, indel): (0, 1, 1)
// for gaps and end-to-end extensions, (-a, b, g) for clipped extensions, whose cost is minus the header's score H.  A clipped
// extension has m = 0 whatever avail is (NB = 2 W + 1), avail is cut at the record of the first piece's text start, the rows beyond
// J + W do not run, and the best cell is the running minimum over all cells (ties: the largest i, then the smallest j).  It ends at
// (a, j_e), the first minimum of row a, if C_e - E <= C*, else at the best cell; the query letters beyond are one 'S' run.
#pragma once

namespace awry {

constexpr int CHAIN_ALIGN_MAX_BAND = 8, CHAIN_ALIGN_MAX_SKEW = 16, CHAIN_ALIGN_MAX_LEN = 1024;
constexpr uint32_t ALN_OK = 0, ALN_SKEW = 1, ALN_BAD_CHAIN = 2;
constexpr int CHAIN_ALIGN_CLASSES = 3;
AWRY_HD constexpr int chain_align_class_nb(int cls) { return cls == 0 ? 9 : cls == 1 ? 17 : 33; }

struct Aln { uint64_t t_begin, t_end; uint32_t edits, status; };  // == awry_aln_t (checked in chain_align_host.h)
struct AlnClip { uint64_t t_begin, t_end; uint32_t edits, status; int32_t score; uint16_t clip_left, clip_right; };  // == awry_aln_clip_t
template <bool CLIP> using AlnOf = std::conditional_t<CLIP, AlnClip, Aln>;
template <bool CLIP> __device__ __forceinline__ AlnOf<CLIP> aln_unaligned(uint64_t tb, uint64_t te, uint32_t status) {
  if constexpr (CLIP) return AlnClip{tb, te, 0, status, 0, 0, 0};
  else return Aln{tb, te, 0, status};
}

// The mode of a launch: end to end (the default), or clipped with the header's weights a, b, g and end bonus E.
struct AlignMode { bool clip = false; int match = 0, mismatch = 1, gap = 1, end_bonus = 0; };
constexpr int CHAIN_CLIP_INF = 1 << 28;  // the clipped mode's +infinity: |cost| <= 64 * 1024 + 8 * 64 stays far below it

// the record of text position t as [lo, hi): awry_get_seq_location's rule, the last record ends at n_text
__device__ __forceinline__ void record_bounds(const DevIndex& ix, uint64_t t, uint64_t n_text, int64_t& lo, int64_t& hi) {
  uint64_t rec[2];
  localise(ix, t < ix.bwt_len ? t : ix.bwt_len - 1, rec);
  lo = ix.nseq ? (int64_t)ix.seq_starts[rec[0]] : 0;
  hi = rec[0] + 1 < ix.nseq ? (int64_t)ix.seq_starts[rec[0] + 1] : (int64_t)n_text;
}

// the direction words of one row: 2 bits per band cell, cell b at bits [2b, 2b + 2) of the row's bit string
template <int NBMAX>
struct ChainAlignTrace {
  using word = std::conditional_t<(NBMAX <= 16), uint32_t, uint64_t>;
  static constexpr int BITS = 8 * (int)sizeof(word);
  static constexpr int NW = (2 * NBMAX + BITS - 1) / BITS;  // 1, 1, 2 words for NBMAX = 9, 17, 33
};

// The pieces of a chain: its members in their order, each clipped on the left by what the pieces before it cover in the query
// or in the text; a member that is covered whole is dropped.  (qe, te) is the running end pair.
struct ChainPieces {
  const Seed* __restrict__ mem;
  uint64_t at, end;
  int64_t qe = 0, te = 0;
  int64_t qb = 0, len = 0, tb = 0;  // the current piece
  bool started = false;
  __device__ __forceinline__ ChainPieces(const Seed* members, uint64_t lo, uint64_t hi) : mem(members), at(lo), end(hi) {}
  __device__ __forceinline__ bool next() {
    while (at < end) {
      const Seed s = mem[at++];
      const int64_t q = s.q_begin, l = s.q_len, t = (int64_t)s.t_pos;
      int64_t o = 0;
      if (started) {
        o = qe - q > te - t ? qe - q : te - t;
        if (o < 0) o = 0;
        if (o >= l) continue;
      }
      qb = q + o; len = l - o; tb = t + o;
      qe = q + l; te = t + l;
      started = true;
      return true;
    }
    return false;
  }
};

// members strictly ascending in q_begin and t_pos, none past L or n_text, at least one; a query of 1 .. max_rows letters
__device__ __forceinline__ bool chain_align_members_ok(const Seed* __restrict__ mem, uint64_t lo, uint64_t hi, uint64_t L, uint64_t n_text,
                                                       uint32_t max_rows) {
  if (hi <= lo || L < 1 || L > (uint64_t)max_rows) return false;
  uint64_t pq = 0, pt = 0;
  for (uint64_t x = lo; x < hi; x++) {
    const Seed s = mem[x];
    if ((uint64_t)s.q_begin + s.q_len > L || s.t_pos > n_text || s.t_pos + s.q_len > n_text) return false;
    if (x > lo && !(s.q_begin > pq && s.t_pos > pt)) return false;
    pq = s.q_begin;
    pt = s.t_pos;
  }
  return true;
}

// One chain per lane, grid-stride: validate the members, walk the pieces for the span and the widest skew, write the record of a
// chain that is not aligned (alns / n_ops non-null: the count pass) and append the others to their class's list:
// lists[cls * m + k], k < list_n[cls] (list_n zeroed by the launcher).  The order inside a list is the order of the atomics;
// every output is indexed by the chain, so it changes nothing.  CLIP: the class and AWRY_ALN_SKEW come from the gaps' skew only (an
// extension needs 2 W + 1 cells), and the records are awry_aln_clip_t.
template <bool CLIP>
__global__ __launch_bounds__(256) void chain_align_classify_kernel(uint64_t n_text, const uint64_t* __restrict__ off, const uint32_t* __restrict__ chain_query,
                                                                   const uint64_t* __restrict__ member_off, const Seed* __restrict__ members, uint64_t m, int W,
                                                                   uint32_t max_rows, AlnOf<CLIP>* __restrict__ alns, uint64_t* __restrict__ n_ops, uint32_t* __restrict__ lists,
                                                                   uint32_t* __restrict__ list_n) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; c < m; c += stride) {
    const uint64_t q = chain_query[c];
    const uint64_t ob = off[q], oe = off[q + 1];
    const uint64_t L = oe > ob ? oe - ob : 0;
    const uint64_t mlo = member_off[c], mhi = member_off[c + 1];
    AlnOf<CLIP> r = aln_unaligned<CLIP>(0, 0, ALN_BAD_CHAIN);
    int64_t skew = 0;
    if (chain_align_members_ok(members, mlo, mhi, L, n_text, max_rows)) {
      ChainPieces p(members, mlo, mhi);
      p.next();
      r.t_begin = (uint64_t)p.tb;
      const int64_t left = p.tb - p.qb;  // avail - a of the left extension
      skew = !CLIP && left < 0 ? -left : 0;
      int64_t pqe = p.qb + p.len, pte = p.tb + p.len;
      while (p.next()) {
        const int64_t mm = (p.tb - pte) - (p.qb - pqe);
        skew = skew > (mm < 0 ? -mm : mm) ? skew : (mm < 0 ? -mm : mm);
        pqe = p.qb + p.len;
        pte = p.tb + p.len;
      }
      r.t_end = (uint64_t)pte;
      const int64_t right = ((int64_t)n_text - pte) - ((int64_t)L - pqe);
      if (!CLIP) skew = skew > -right ? skew : -right;
      r.status = skew > CHAIN_ALIGN_MAX_SKEW ? ALN_SKEW : ALN_OK;
    }
    if (r.status != ALN_OK) {
      if (alns) alns[c] = r;
      if (n_ops) n_ops[c] = 0;
      continue;
    }
    const int nb = (int)skew + 2 * W + 1;
    const int cls = nb <= chain_align_class_nb(0) ? 0 : nb <= chain_align_class_nb(1) ? 1 : 2;
    const uint32_t k = atomicAdd(&list_n[cls], 1u);
    lists[(uint64_t)cls * m + k] = (uint32_t)c;
  }
}

// The chains of one class, one per lane, grid-stride over list[0 .. *list_n).  The lane walks the chain left to right: left
// extension, then piece and gap in turn, then the right extension, through ONE copy of the row update (the segment's kind only
// sets where x and y are read and where the alignment ends).  Only segment rows run the table; row i of a segment stores its
// direction words at trace[(qpos * NW + w) * lanes_in_grid + lane], qpos the query letter of the row, so a wave's stores are
// contiguous and no two segments of a chain share a row.  The left extension works on reversed strings: its traceback from
// (a, j*) meets the operations in query order and emits them as it goes.  A gap or right extension's traceback meets them last to
// first: it rewrites word 0 of each row it leaves as (the row's '=' / 'X' / 'I') | (the 'D's after it) << 2, and a forward walk
// over the rows then emits them.  Runs are merged over the whole script as they are emitted.
// FILL = false: the count pass -- alns[c] and n_ops[c]; FILL = true: the runs at cigar[cigar_off[c] .. cigar_off[c + 1]).
// tally (nullable): [0] += chains aligned, [1] += table cells inside band and table.
// CLIP = true: the clipped mode (ix gives the record bounds, md the weights); the cells are signed, the left extension emits its
// 'S' run before its traceback and the right extension after its forward walk, and score and edits are counted as the operations
// are emitted, so that they are the script's by construction.  CLIP = false reads neither ix nor md: the weights are constants.
template <int A, int NBMAX, bool FILL, bool CLIP>
__global__ __launch_bounds__(256) void chain_align_kernel(const uint8_t* __restrict__ text8, uint64_t n_text, const uint8_t* __restrict__ ascii,
                                                          const uint64_t* __restrict__ off, const uint32_t* __restrict__ chain_query,
                                                          const uint64_t* __restrict__ member_off, const Seed* __restrict__ members,
                                                          const uint32_t* __restrict__ list, const uint32_t* __restrict__ list_n, int W,
                                                          typename ChainAlignTrace<NBMAX>::word* trace, AlnOf<CLIP>* __restrict__ alns,
                                                          uint64_t* __restrict__ n_ops, const uint64_t* __restrict__ cigar_off, uint32_t* __restrict__ cigar,
                                                          unsigned long long* __restrict__ tally, DevIndex ix, AlignMode md) {
  using TR = ChainAlignTrace<NBMAX>;
  using TW = typename TR::word;
  using cell = std::conditional_t<CLIP, int32_t, uint32_t>;  // a table cell: a cost, signed where a match earns
  constexpr cell CINF = CLIP ? (cell)CHAIN_CLIP_INF : (cell)ALIGN_INF;
  constexpr int NW = TR::NW, BITS = TR::BITS;
  constexpr uint32_t S = edit_symbols(A);
  __shared__ uint8_t lut[256];
  lut[threadIdx.x] = (uint8_t)(threadIdx.x >= 128 ? 0xFF : index_of_ascii(A, (uint8_t)threadIdx.x));
  __syncthreads();
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x, lane = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t* __restrict__ text = reinterpret_cast<const uint64_t*>(text8);
  const uint64_t count = *list_n;
  unsigned long long t_chains = 0, t_cells = 0;
  for (uint64_t at = lane; at < count; at += stride) {
    const uint64_t c = list[at];
    const uint64_t q = chain_query[c];
    const uint64_t q0 = off[q];
    const int L = (int)(off[q + 1] - q0);  // 1 .. max_rows of the launch: the classify kernel has checked it
    uint64_t word = 0, word_at = ~0ull;
    auto symbol = [&](int64_t p) -> uint32_t {  // T[p], 0 outside the text
      if ((uint64_t)p >= n_text) return 0u;
      if (((uint64_t)p >> 3) != word_at) { word_at = (uint64_t)p >> 3; word = text[word_at]; }
      return (uint32_t)(word >> (8 * ((uint64_t)p & 7))) & 0xFFu;
    };
    ByteStream qbytes(ascii);
    // the run writer: runs are merged over the whole script
    uint32_t run_op = 0, run_len = 0;
    uint64_t nruns = 0;
    const uint64_t out_at = FILL ? cigar_off[c] : 0, out_cap = FILL ? cigar_off[c + 1] - out_at : 0;
    auto flush = [&]() {
      if (run_len) {
        if (FILL && nruns < out_cap) cigar[out_at + nruns] = run_len << 4 | run_op;
        nruns++;
      }
    };
    int32_t score = 0;    // CLIP: a #'=' - b #'X' - g (#'I' + #'D') of what has been emitted
    uint32_t edits = 0;   // CLIP: #'X' + #'I' + #'D' of what has been emitted; else the pieces' 'X's and the segments' costs
    auto emit = [&](uint32_t op, uint32_t cnt) {
      if (!cnt) return;
      if (op != run_op || (CLIP && op == 4u)) { flush(); run_op = op; run_len = 0; }  // (an 'S' run merges with nothing)
      run_len += cnt;
      if constexpr (CLIP) {
        if (op == 7u) score += md.match * (int32_t)cnt;
        else if (op != 4u) { edits += cnt; score -= (op == 8u ? md.mismatch : md.gap) * (int32_t)cnt; }
      }
    };
    ChainPieces p(members, member_off[c], member_off[c + 1]);
    p.next();
    const int64_t t_first = p.tb;
    int64_t t_begin = p.tb, t_end = p.tb, pqe = 0, pte = 0;
    int64_t rec_lo = 0, rec_hi = (int64_t)n_text;  // what an extension may read: the text, CLIP: the first piece's record
    if constexpr (CLIP) record_bounds(ix, (uint64_t)p.tb, n_text, rec_lo, rec_hi);
    uint32_t clip_left = 0, clip_right = 0;
    bool sane = true;
    for (int kind = 0; sane;) {  // 0: the left extension and the first piece; 1: a gap and its piece; 2: the right extension
      // ---- the segment: row i reads query letter xq + xs * i, column j reads T[ty + ts * (j - 1)] ----
      int a, J, msk, end_j;
      int64_t xq, ty;
      int xs;
      if (kind == 0) {
        a = (int)p.qb;
        const int64_t avail = p.tb - rec_lo;
        msk = !CLIP && avail < a ? (int)(avail - a) : 0;
        J = avail < a + W ? (int)avail : a + W;
        end_j = -1;
        xq = p.qb; xs = -1; ty = p.tb - 1;
      } else if (kind == 1) {
        a = (int)(p.qb - pqe);
        J = (int)(p.tb - pte);
        msk = J - a;
        end_j = J;
        xq = pqe - 1; xs = 1; ty = pte;
      } else {
        a = L - (int)pqe;
        const int64_t avail = rec_hi > pte ? rec_hi - pte : 0;
        msk = !CLIP && avail < a ? (int)(avail - a) : 0;
        J = avail < a + W ? (int)avail : a + W;
        end_j = -1;
        xq = pqe - 1; xs = 1; ty = pte;
      }
      const int ts = xs;
      if (a > 0 || kind == 1) {
        const int lo = (msk < 0 ? msk : 0) - W, hi = (msk > 0 ? msk : 0) + W, NB = hi - lo + 1;
        if (NB > NBMAX) { sane = false; break; }  // (never: the class holds the chain's widest segment)
        const bool local = CLIP && kind != 1;  // a clipped extension: weights (-a, b, g), the best cell tracked, rows up to J + W
        const cell wm = local ? (cell)-md.match : (cell)0, wx = local ? (cell)md.mismatch : (cell)1, wg = local ? (cell)md.gap : (cell)1;
        const int rows = local && J + W < a ? J + W : a;
        cell best = 0;                 // the running minimum over all cells: (0, 0) to begin with
        int best_i = 0, best_b = -lo;
        cell cc[NBMAX];      // cc[b] = C[i][i + b + lo]
        uint32_t tw[NBMAX];  // tw[b] = y of column i + b + lo, the symbol cell b of row i compares
#pragma unroll
        for (int b = 0; b < NBMAX; b++) {
          const int j = b + lo;
          cc[b] = b < NB && j >= 0 && j <= J ? (cell)j * wg : CINF;  // row 0
          tw[b] = j >= 0 ? symbol(ty + (int64_t)ts * j) : 0u;        // row 1: column j + 1
        }
        if (tally) t_cells += (unsigned long long)((hi < J ? hi : J) + 1);
        for (int i = 1; i <= rows; i++) {
          if (i > 1) {
#pragma unroll
            for (int b = 0; b + 1 < NBMAX; b++) tw[b] = tw[b + 1];
            const int jn = i + NBMAX - 1 + lo - 1;  // the 0-based y index under cell NBMAX - 1
            tw[NBMAX - 1] = jn >= 0 ? symbol(ty + (int64_t)ts * jn) : 0u;
          }
          const int64_t qpos = xq + (int64_t)xs * i;
          const uint32_t qs = lut[qbytes[q0 + (uint64_t)qpos]];
          TW dirs[NW];
#pragma unroll
          for (int w = 0; w < NW; w++) dirs[w] = 0;
          cell left = CINF;
#pragma unroll
          for (int b = 0; b < NBMAX; b++) {
            const int j = i + b + lo;
            const uint32_t neq = tw[b] == qs && tw[b] - 1u < S ? 0u : 1u;
            const cell dg = cc[b] + (neq ? wx : wm), up = (b + 1 < NBMAX ? cc[b + 1] : CINF) + wg, lf = left + wg;
            cell v = dg < up ? dg : up;
            v = v < lf ? v : lf;
            uint32_t dir = dg == v ? neq : (up == v ? 2u : 3u);
            if (j == 0) { v = (cell)i * wg; dir = 2u; }  // column 0: only 'I' leads back
            const bool outside = b >= NB || j < 0 || j > J;
            if (outside) v = CINF;
            if constexpr (CLIP) {  // ties: the largest i, then the smallest j -- rows and cells come in that order
              if (local && !outside && (v < best || (v == best && best_i != i))) { best = v; best_i = i; best_b = b; }
            }
            cc[b] = v;
            left = v;
            dirs[(2 * b) / BITS] |= (TW)dir << ((2 * b) % BITS);
          }
#pragma unroll
          for (int w = 0; w < NW; w++) trace[((uint64_t)qpos * NW + w) * stride + lane] = dirs[w];
          if (tally) {
            const int c0 = i + lo > 0 ? i + lo : 0, c1 = i + hi < J ? i + hi : J;
            if (c1 >= c0) t_cells += (unsigned long long)(c1 - c0 + 1);
          }
        }
        // ---- where it ends ----
        cell cost = CINF;
        int b = 0;
        if (end_j < 0) {
#pragma unroll
          for (int x = 0; x < NBMAX; x++)
            if (cc[x] < cost) { cost = cc[x]; b = x; }  // the first minimum: the smallest end column
        } else {
          b = end_j - a - lo;
#pragma unroll
          for (int x = 0; x < NBMAX; x++)
            if (x == b) cost = cc[x];
        }
        int i = a;
        if constexpr (CLIP) {
          // cc is row `rows`: row a iff it has a cell.  It ends there unless the best cell beats it by more than the end bonus.
          if (local && (rows < a || cost - (cell)md.end_bonus > best)) { cost = best; i = best_i; b = best_b; }
          if (cost >= CINF / 2) { sane = false; break; }  // (never)
          if (kind == 0) clip_left = (uint32_t)(a - i);
        } else {
          if (cost >= CINF) { sane = false; break; }  // (never: every cell inside band and table is reachable)
          edits += cost;
        }
        const int i_end = i;
        int j = i + b + lo;
        if (kind == 0) { t_begin = p.tb - j; emit(4u, clip_left); }
        if (kind == 2) t_end = pte + j;
        // ---- the traceback ----
        uint32_t after = 0;  // 'D's met since the last row was left (forward kinds)
        int64_t have = -1;   // the trace word in `dw`: row * NW + w
        TW dw = 0;
        while (i > 0) {
          if ((uint32_t)b >= (uint32_t)NB || j < 0) { sane = false; break; }  // (never on a consistent table)
          const int64_t qpos = xq + (int64_t)xs * i;
          const int64_t need = qpos * NW + (2 * b) / BITS;
          if (need != have) { have = need; dw = trace[(uint64_t)need * stride + lane]; }
          const uint32_t dir = (uint32_t)(dw >> ((2 * b) % BITS)) & 3u;
          if (dir == 3u) {
            if (kind == 0) emit(2u, 1u); else after++;
            j--; b--;
            continue;
          }
          if (kind == 0) {
            emit(align_bam_op(dir), 1u);
          } else {
            trace[(uint64_t)qpos * NW * stride + lane] = (TW)(dir | after << 2);
            after = 0;
            have = -1;
          }
          i--;
          if (dir <= 1u) j--; else b++;
        }
        if (!sane) break;
        // row 0: only 'D' leads back
        if (kind == 0) {
          emit(2u, (uint32_t)j);
        } else {
          emit(2u, (uint32_t)j);
          for (int r = 1; r <= i_end; r++) {
            const TW w0 = trace[(uint64_t)(xq + r) * NW * stride + lane];
            emit(align_bam_op((uint32_t)w0 & 3u), 1u);
            emit(2u, (uint32_t)(w0 >> 2));
          }
          if (CLIP && kind == 2) { clip_right = (uint32_t)(a - i_end); emit(4u, clip_right); }
        }
      }
      if (kind == 2) break;
      // ---- the piece: a diagonal run, '=' or 'X' letter by letter ----
      for (int64_t x = 0; x < p.len; x++) {
        const uint32_t qs = lut[qbytes[q0 + (uint64_t)(p.qb + x)]], tsym = symbol(p.tb + x);
        const uint32_t neq = tsym == qs && tsym - 1u < S ? 0u : 1u;
        if (!CLIP) edits += neq;
        emit(neq ? 8u : 7u, 1u);
      }
      pqe = p.qb + p.len;
      pte = p.tb + p.len;
      t_end = pte;
      kind = p.next() ? 1 : 2;
    }
    flush();
    if (!sane) {  // (never) the record of a chain that is not aligned, and no runs
      if (!FILL) { alns[c] = aln_unaligned<CLIP>((uint64_t)t_first, (uint64_t)pte, ALN_BAD_CHAIN); n_ops[c] = 0; }
      continue;
    }
    if (!FILL) {
      if constexpr (CLIP) alns[c] = AlnClip{(uint64_t)t_begin, (uint64_t)t_end, edits, ALN_OK, score, (uint16_t)clip_left, (uint16_t)clip_right};
      else alns[c] = Aln{(uint64_t)t_begin, (uint64_t)t_end, edits, ALN_OK};
      n_ops[c] = nruns;
    }
    t_chains++;
  }
  if (tally) {
    if (t_chains) atomicAdd(&tally[0], t_chains);
    if (t_cells) atomicAdd(&tally[1], t_cells);
  }
}

// chain k of query i (k < n_chains[i]) is taken iff k < max_alignments: the count per query as scan input
__global__ __launch_bounds__(256) void chain_align_take_kernel(const uint64_t* __restrict__ n_chains, uint64_t n, uint64_t max_alignments,
                                                               uint64_t* __restrict__ taken) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) taken[i] = n_chains[i] < max_alignments ? n_chains[i] : max_alignments;
}

// One query per lane: its first aln_off[i + 1] - aln_off[i] chains become the selected chains aln_off[i] ..: their query, their
// record, and their member count as scan input.
__global__ __launch_bounds__(256) void chain_align_select_kernel(const uint64_t* __restrict__ chain_off, const Chain* __restrict__ chains,
                                                                 const uint64_t* __restrict__ aln_off, uint64_t n,
                                                                 uint32_t* __restrict__ sel_query, Chain* __restrict__ sel_chains,
                                                                 uint64_t* __restrict__ sel_member_cnt) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const uint64_t lo = aln_off[i], cnt = aln_off[i + 1] - lo, from = chain_off[i];
    for (uint64_t k = 0; k < cnt; k++) {
      const Chain ch = chains[from + k];
      sel_query[lo + k] = (uint32_t)i;
      sel_chains[lo + k] = ch;
      sel_member_cnt[lo + k] = ch.n_seeds;
    }
  }
}

// The members of the selected chains, compacted.  The members of a query's chains lie back to back from member_off[i], in chain
// order, so those of its first chains are a prefix of that range.
__global__ __launch_bounds__(256) void chain_align_gather_kernel(const uint64_t* __restrict__ member_off,
                                                                 const Seed* __restrict__ members, const uint64_t* __restrict__ aln_off,
                                                                 const uint64_t* __restrict__ sel_member_off, uint64_t n, Seed* __restrict__ sel_members) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const uint64_t lo = aln_off[i], hi = aln_off[i + 1];
    if (hi <= lo) continue;
    const uint64_t cnt = sel_member_off[hi] - sel_member_off[lo], from = member_off[i], to = sel_member_off[lo];
    for (uint64_t x = 0; x < cnt; x++) sel_members[to + x] = members[from + x];
  }
}

}  // namespace awry
