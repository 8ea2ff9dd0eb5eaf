// kernels_chain.hip.h -- colinear chaining of located seeds: sort, a windowed dynamic programme and minimap2's backtrack, one query
// per GROUP of lanes (a whole wave, or 16 lanes: four queries per wave).
// Included by kernels.hip.h after kernels_align.hip.h (it uses localise, tally_add).
//
// No counterpart in the reference.  The definition, as include/awry_hip.h states it: the N seeds (q_begin, q_len, t_pos) of a query,
// sorted by (t_pos, q_begin, q_len, input index); for j < i, i - j <= lookback, with dq = q_begin_i - q_begin_j, dt = t_pos_i -
// t_pos_j, g = |dq - dt|: j may precede i iff rec_j == rec_i, 0 < dq <= max_gap, 0 < dt <= max_gap, g <= max_skew;
//     gain(j, i) = min(q_len_i, dq, dt) - g
//     f_i = max(q_len_i, max over admissible j of f_j + gain(j, i));  p_i = the LARGEST such j that attains f_i > q_len_i
// then seeds are visited in descending f (ties: ascending index); an unvisited seed ends a chain, which is walked along p until
// there is no predecessor (base 0) or a used one (base = its f, not a member); score = f_end - base, reported iff >= min_score.
//
// Mapping.  The recurrence is serial in i and at most 64 wide in j: lane l of the group evaluates predecessor i - 1 - l from the
// group's tile (LDS while N fits it, else the group's slab of the stream's workspace), the group reduces the candidate scores to
// their maximum with DPP steps inside a row of 16 lanes (quad_perm, row_ror) and two cross-row shuffles for the 64-lane group, a
// ballot names the lowest lane -- the largest j -- that holds it, and lane 0 writes f_i and p_i.  Both sorts are bitonic networks
// over the same tile.  Every pass recomputes the chains: the fill pass keeps nothing of the count pass, as the anchor and SMEM
// kernels do, so any number of launches may lie between the two.
#pragma once

namespace awry {

struct Seed { uint32_t q_begin, q_len; uint64_t t_pos; };                               // == awry_seed_t (checked in chain_host.h)
struct Chain { uint32_t score, n_seeds, q_begin, q_end; uint64_t t_begin, t_end; };   // == awry_chain_t
struct ChainParams { uint32_t max_seeds, lookback, max_gap, max_skew, min_score; };

constexpr uint8_t Q_SEED_CAP = 8;  // AWRY_Q_SEED_CAP: the query has more seeds than max_seeds
constexpr int CHAIN_MAX_SEEDS = 4096, CHAIN_MAX_LOOKBACK = 64;
constexpr uint32_t CHAIN_NONE = 0x7FFFFFFFu, CHAIN_USED = 0x80000000u;  // p: no predecessor; the seed belongs to a walked chain
// bytes of the working set per seed: t_pos and the backtrack key (8 each), q_begin, q_len, f (the input index while sorting), rec, p
constexpr int CHAIN_SEED_BYTES = 36;
// seeds of a query a group keeps in LDS: 36 KiB per block of 256 lanes in both instantiations, four blocks per CU
template <int G> struct ChainTile { static constexpr int value = G == 64 ? 256 : 64; };

// the working set of one query over `cap` slots (a power of two) at `base`
struct ChainSet {
  uint64_t* tpos; uint64_t* bkey; uint32_t* qb; uint32_t* ql; uint32_t* f; uint32_t* rec; uint32_t* p;
  __device__ __forceinline__ ChainSet(char* base, uint32_t cap) {
    tpos = reinterpret_cast<uint64_t*>(base);
    bkey = tpos + cap;
    qb = reinterpret_cast<uint32_t*>(bkey + cap);
    ql = qb + cap; f = ql + cap; rec = f + cap; p = rec + cap;
  }
};

// the lanes of a group run in lockstep (they share a wave); what one wrote, the others read after this
__device__ __forceinline__ void chain_sync() {
  __threadfence_block();
  __builtin_amdgcn_wave_barrier();
}

// maximum over the group's lanes, in every lane: inside a row of 16 lanes by DPP, across the rows of a wave by shuffles
template <int G>
__device__ __forceinline__ uint32_t group_max(uint32_t v) {
  v = max(v, (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0xB1, 0xF, 0xF, true));   // quad_perm [1,0,3,2]
  v = max(v, (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x4E, 0xF, 0xF, true));   // quad_perm [2,3,0,1]
  v = max(v, (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x124, 0xF, 0xF, true));  // row_ror:4
  v = max(v, (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x128, 0xF, 0xF, true));  // row_ror:8
  if (G == 64) {
    v = max(v, (uint32_t)__shfl_xor((int)v, 16, 64));
    v = max(v, (uint32_t)__shfl_xor((int)v, 32, 64));
  }
  return v;
}

// bitonic network over slots [0, S), S a power of two, ascending by the strict total order less(a, b) of slot contents
template <int G, class Less, class Swap>
__device__ __forceinline__ void group_bitonic(uint32_t S, uint32_t gl, Less less, Swap swap) {
  for (uint32_t k = 2; k <= S; k <<= 1)
    for (uint32_t j = k >> 1; j > 0; j >>= 1) {
      for (uint32_t t = gl; t < (S >> 1); t += G) {
        const uint32_t a = ((t & ~(j - 1)) << 1) | (t & (j - 1)), b = a | j;
        if ((a & k) == 0 ? less(b, a) : less(a, b)) swap(a, b);
      }
      chain_sync();
    }
}

// the record of a seed: what awry_get_seq_location answers for t_pos (a position past the text: the last record)
__device__ __forceinline__ uint32_t chain_record(const DevIndex& ix, uint64_t g) {
  uint64_t out[2];
  localise(ix, g < ix.bwt_len ? g : ix.bwt_len - 1, out);
  return (uint32_t)out[0];
}

// One query of N <= cap seeds on the group's lanes (gl = lane in the group).  Lane 0 leaves the counts in nch / nmem and, FILL,
// the records: chain c at chains[c] while c < chain_room, its members first to last at members[...] below member_room.
template <int G, int FILL>
__device__ __forceinline__ void chain_query(const DevIndex& ix, char* base, uint32_t cap, const Seed* __restrict__ seeds, uint32_t N,
                                            const ChainParams& P, uint32_t gl, uint64_t& nch, uint64_t& nmem, Chain* __restrict__ chains,
                                            uint64_t chain_room, Seed* __restrict__ members, uint64_t member_room) {
  const ChainSet w(base, cap);
  uint32_t S = 1;
  while (S < N) S <<= 1;
  for (uint32_t t = gl; t < S; t += G) {  // slots past the seeds hold the order's maximum
    const bool in = t < N;
    Seed sd{~0u, ~0u, ~0ull};
    if (in) sd = seeds[t];
    w.tpos[t] = sd.t_pos; w.qb[t] = sd.q_begin; w.ql[t] = sd.q_len; w.f[t] = t;
  }
  chain_sync();
  group_bitonic<G>(S, gl,
      [&](uint32_t a, uint32_t b) {
        const uint64_t ta = w.tpos[a], tb = w.tpos[b];
        if (ta != tb) return ta < tb;
        const uint32_t qa = w.qb[a], qb = w.qb[b];
        if (qa != qb) return qa < qb;
        const uint32_t la = w.ql[a], lb = w.ql[b];
        if (la != lb) return la < lb;
        return w.f[a] < w.f[b];
      },
      [&](uint32_t a, uint32_t b) {
        const uint64_t t = w.tpos[a]; w.tpos[a] = w.tpos[b]; w.tpos[b] = t;
        uint32_t x = w.qb[a]; w.qb[a] = w.qb[b]; w.qb[b] = x;
        x = w.ql[a]; w.ql[a] = w.ql[b]; w.ql[b] = x;
        x = w.f[a]; w.f[a] = w.f[b]; w.f[b] = x;
      });
  for (uint32_t t = gl; t < N; t += G) w.rec[t] = chain_record(ix, w.tpos[t]);
  chain_sync();
  // the dynamic programme: serial in i, the group's lanes over the predecessors
  for (uint32_t i = 0; i < N; i++) {
    const uint64_t ti = w.tpos[i];
    const uint32_t qi = w.qb[i], li = w.ql[i], ri = w.rec[i];
    uint32_t key = 0;
    if (gl < P.lookback && gl < i) {
      const uint32_t j = i - 1 - gl;
      const int64_t dq = (int64_t)qi - (int64_t)w.qb[j];
      const uint64_t dt = ti - w.tpos[j];
      if (w.rec[j] == ri && dq > 0 && dq <= (int64_t)P.max_gap && dt > 0 && dt <= (uint64_t)P.max_gap) {
        int64_t g = dq - (int64_t)dt;
        g = g < 0 ? -g : g;
        if (g <= (int64_t)P.max_skew) {
          const int64_t cand = (int64_t)w.f[j] + min(min((int64_t)li, dq), (int64_t)dt) - g;
          if (cand > (int64_t)li) key = (uint32_t)cand;
        }
      }
    }
    const uint32_t best = group_max<G>(key);
    uint64_t holders = __ballot(best != 0 && key == best);
    if (G < 64) holders = (holders >> (threadIdx.x & 63u & ~(uint32_t)(G - 1))) & ((1ull << (G & 63)) - 1);
    if (gl == 0) {
      w.f[i] = best ? best : li;
      w.p[i] = best ? i - 1 - (uint32_t)__builtin_ctzll(holders) : CHAIN_NONE;
    }
    chain_sync();
  }
  // visit order: descending f, ascending index
  for (uint32_t t = gl; t < S; t += G) w.bkey[t] = t < N ? ((uint64_t)(~w.f[t]) << 32) | t : ~0ull;
  chain_sync();
  group_bitonic<G>(S, gl, [&](uint32_t a, uint32_t b) { return w.bkey[a] < w.bkey[b]; },
                   [&](uint32_t a, uint32_t b) { const uint64_t t = w.bkey[a]; w.bkey[a] = w.bkey[b]; w.bkey[b] = t; });
  if (gl == 0) {  // the serial walk
    uint64_t c = 0, m = 0;
    for (uint32_t r = 0; r < N; r++) {
      const uint32_t e = (uint32_t)w.bkey[r];
      if (w.p[e] & CHAIN_USED) continue;
      uint32_t u = e, cnt = 0, first = e, qend = 0;
      uint64_t tend = 0, fbase = 0;
      for (;;) {
        const uint32_t pu = w.p[u];
        w.p[u] = pu | CHAIN_USED;
        cnt++;
        first = u;
        const uint32_t len = w.ql[u], qe = w.qb[u] + len;
        const uint64_t te = w.tpos[u] + len;
        qend = cnt == 1 || qe > qend ? qe : qend;
        tend = cnt == 1 || te > tend ? te : tend;
        if (pu == CHAIN_NONE) break;
        if (w.p[pu] & CHAIN_USED) { fbase = w.f[pu]; break; }
        u = pu;
      }
      const int64_t score = (int64_t)w.f[e] - (int64_t)fbase;
      if (score < (int64_t)P.min_score) continue;
      if (FILL) {
        if (c < chain_room) chains[c] = Chain{(uint32_t)score, cnt, w.qb[first], qend, w.tpos[first], tend};
        u = e;
        for (uint32_t k = 0; k < cnt; k++) {  // members: walked last to first, written first to last
          const uint64_t at = m + (cnt - 1 - k);
          if (at < member_room) members[at] = Seed{w.qb[u], w.ql[u], w.tpos[u]};
          u = w.p[u] & ~CHAIN_USED;
        }
      }
      c++;
      m += cnt;
    }
    nch = c;
    nmem = m;
  }
  chain_sync();  // the tile is free for the group's next query
}

// n queries; query q has the seeds [seed_off[q], seed_off[q+1]) of `seeds`.  FILL 0: the count pass -> n_chains[q], n_members[q]
// (u64); FILL 1: chains of q at chains[chain_off[q] ...), their members back to back at members[member_off[q] ...), never a slot
// at or beyond the next query's offset.  status (nullable): Q_OK, or Q_SEED_CAP for a query of more than max_seeds seeds, which
// has no chains.  slabs: slab_cap * CHAIN_SEED_BYTES bytes per group of the grid, for queries beyond the LDS tile (slab_cap a
// power of two >= max_seeds, or 0 when max_seeds fits the tile).  tally (nullable): += {seeds chained, predecessor pairs
// evaluated, chains reported}
template <int G, int FILL>
__global__ __launch_bounds__(256) void chain_kernel(DevIndex ix, const uint64_t* __restrict__ seed_off, const Seed* __restrict__ seeds, uint64_t n,
                                                    ChainParams P, uint64_t* __restrict__ n_chains, uint64_t* __restrict__ n_members,
                                                    const uint64_t* __restrict__ chain_off, const uint64_t* __restrict__ member_off,
                                                    Chain* __restrict__ chains, Seed* __restrict__ members, uint8_t* __restrict__ status,
                                                    char* __restrict__ slabs, uint32_t slab_cap, unsigned long long* tally) {
  constexpr int GROUPS = 256 / G, T = ChainTile<G>::value;
  __shared__ __attribute__((aligned(16))) char tile[GROUPS * T * CHAIN_SEED_BYTES];
  const uint32_t group = threadIdx.x / G, gl = threadIdx.x % G;
  const uint64_t gid = (uint64_t)blockIdx.x * GROUPS + group, ngroups = (uint64_t)gridDim.x * GROUPS;
  for (uint64_t q = gid; q < n; q += ngroups) {
    const uint64_t s0 = seed_off[q], s1 = seed_off[q + 1];
    const bool capped = s1 < s0 || s1 - s0 > (uint64_t)P.max_seeds;
    const uint32_t N = capped ? 0 : (uint32_t)(s1 - s0);
    uint64_t nch = 0, nmem = 0, c0 = 0, c1 = 0, m0 = 0, m1 = 0;
    if (FILL) { c0 = chain_off[q]; c1 = chain_off[q + 1]; m0 = member_off[q]; m1 = member_off[q + 1]; }
    const uint64_t chain_room = c1 > c0 ? c1 - c0 : 0, member_room = m1 > m0 ? m1 - m0 : 0;
    if (N <= (uint32_t)T)
      chain_query<G, FILL>(ix, tile + (size_t)group * T * CHAIN_SEED_BYTES, T, seeds + s0, N, P, gl, nch, nmem, chains + c0, chain_room, members + m0,
                           member_room);
    else if (N <= slab_cap)
      chain_query<G, FILL>(ix, slabs + (size_t)gid * slab_cap * CHAIN_SEED_BYTES, slab_cap, seeds + s0, N, P, gl, nch, nmem, chains + c0, chain_room,
                           members + m0, member_room);
    if (gl == 0) {
      if (!FILL) { n_chains[q] = nch; n_members[q] = nmem; }
      if (status) status[q] = capped ? Q_SEED_CAP : Q_OK;
      if (tally) {
        const uint64_t lb = P.lookback, full = N > lb ? N - lb : 0, ramp = N - full;  // sum over i of min(i, lookback)
        tally_add(tally, 0, N);
        tally_add(tally, 1, ramp * (ramp ? ramp - 1 : 0) / 2 + full * lb);
        tally_add(tally, 2, nch);
      }
    }
  }
}

// located hits of SMEM records -> seeds: hit h belongs to the record s with hit_off[s] <= h < hit_off[s+1]
__global__ __launch_bounds__(256) void chain_expand_kernel(const Anchor* __restrict__ recs, const uint64_t* __restrict__ hit_off, uint64_t nrec,
                                                           const uint64_t* __restrict__ gpos, uint64_t nhits, Seed* __restrict__ seeds) {
  for (uint64_t h = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; h < nhits; h += (uint64_t)gridDim.x * blockDim.x) {
    uint64_t a = 0, z = nrec;  // the largest s with hit_off[s] <= h
    while (z - a > 1) { const uint64_t mid = (a + z) >> 1; if (hit_off[mid] <= h) a = mid; else z = mid; }
    const Anchor r = recs[a];
    seeds[h] = Seed{r.q_begin, r.q_len, gpos[h]};
  }
}
// per-query seed offsets: seed_off[q] = hit_off[rec_off[q]], q = 0..n
__global__ __launch_bounds__(256) void chain_seed_off_kernel(const uint64_t* __restrict__ rec_off, const uint64_t* __restrict__ hit_off, uint64_t n1,
                                                             uint64_t* __restrict__ seed_off) {
  for (uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; q < n1; q += (uint64_t)gridDim.x * blockDim.x) seed_off[q] = hit_off[rec_off[q]];
}

}  // namespace awry
