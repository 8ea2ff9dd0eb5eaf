// chain_host.h -- the chunk driver of chaining: the SMEM locate flow of anchor_host.h, then seeds, the chain count pass, two scans,
// the fill pass and the copy-out
// A part of awry_hip.hip (one translation unit): included there, in order, and not on its own.
#pragma once

namespace {

// ---- chaining (kernels_chain.hip.h) -----------------------------------------------------------------------------------

static_assert(sizeof(Seed) == sizeof(awry_seed_t) && sizeof(awry_seed_t) == 16 && offsetof(Seed, t_pos) == offsetof(awry_seed_t, t_pos) &&
                  sizeof(Chain) == sizeof(awry_chain_t) && sizeof(awry_chain_t) == 32 && offsetof(Chain, q_end) == offsetof(awry_chain_t, q_end) &&
                  offsetof(Chain, t_begin) == offsetof(awry_chain_t, t_begin) && offsetof(Chain, t_end) == offsetof(awry_chain_t, t_end),
              "the kernels write awry_seed_t and awry_chain_t records");
static_assert(Q_SEED_CAP == AWRY_Q_SEED_CAP && CHAIN_MAX_SEEDS == AWRY_CHAIN_MAX_SEEDS && CHAIN_MAX_LOOKBACK == AWRY_CHAIN_MAX_LOOKBACK,
              "the kernels' limits are the header's");

ChainParams chain_params(uint32_t max_seeds, uint32_t lookback, uint32_t max_gap, uint32_t max_skew, uint32_t min_score) {
  if (max_seeds < 1 || max_seeds > (uint32_t)CHAIN_MAX_SEEDS) throw ArgError("max_seeds must be in 1..4096 (AWRY_CHAIN_MAX_SEEDS)");
  if (lookback < 1 || lookback > (uint32_t)CHAIN_MAX_LOOKBACK) throw ArgError("lookback must be in 1..64 (AWRY_CHAIN_MAX_LOOKBACK)");
  if (max_gap < 1) throw ArgError("max_gap must be at least 1");
  if (min_score < 1) throw ArgError("min_score must be at least 1");
  return ChainParams{max_seeds, lookback, max_gap, max_skew, min_score};
}

void require_chain_index(uint64_t bwt_len) {
  if (bwt_len >= (1ull << 32)) throw ArgError("chaining needs an index with bwt_len < 2^32");
}

struct ChainHits {  // one shard's result, in query order
  std::vector<uint64_t> n_chains;  // per query
  std::vector<uint8_t> status;     // per query: Q_OK or Q_SEED_CAP
  std::vector<awry_chain_t> chains;
  std::vector<awry_seed_t> members;
};

// what a chunk's fill pass leaves on the device, for a driver that goes on there (chain_align_host.h) instead of copying it out
struct ChainOnDevice {
  const ChunkBuffers& cb;  // the chunk's queries
  Shard c;
  const uint64_t *n_chains, *chain_off, *member_off;  // per query
  const Chain* chains;
  const Seed* members;
  uint64_t nchains, nmembers;
  const uint8_t* status;  // per query: Q_OK or Q_SEED_CAP
};
using ChainSink = std::function<void(Replica&, const ChainOnDevice&)>;  // returns with the stream synchronised

template <class K, class... Args>
void chain_launch(Replica& r, hipStream_t s, uint64_t items, K kernel, Args... args) {
  hipLaunchKernelGGL(kernel, dim3(grid_for(r, items, 256)), dim3(256), 0, s, args...);
  HIP_CHECK(hipGetLastError());
}

// SMEM count pass, scan, fill pass, ranges, scan of the located counts and locate (anchor_chunk's flow, text positions only); then
// one seed per located hit, the chain count pass, the scans of chains and members, the fill pass.  false: the chunk's located
// hits exceed the capacity and it holds more than one query -- nothing appended.  With a sink, the chunk's chains and members go
// to it, on the device, and nothing is appended to `out`.  both_strands (with a sink): the chunk's reads are uploaded once and
// expanded on the device into the doubled batch (launch_strand_expand: query 2i = read i, query 2i + 1 = its reverse complement);
// everything after that, the sink's view included, is over the 2 (c.hi - c.lo) queries, a rejected query is reported under its
// read's index, and the capacity test counts reads, so a read's two strands are never split.
bool chain_chunk(Replica& r, const uint8_t* qbytes, const uint64_t* qoff, Shard c, uint32_t min_len, uint64_t max_hits, const ChainParams& P,
                 bool want_members, ChainHits& out, const ChainSink* sink = nullptr, bool both_strands = false) {
  const hipStream_t s = r.stream;
  const uint64_t nreads = c.hi - c.lo, n = both_strands ? 2 * nreads : nreads;
  for (uint64_t i = c.lo; i < c.hi; i++)
    if (qoff[i + 1] >= qoff[i] && qoff[i + 1] - qoff[i] >= (1ull << 31)) throw ArgError("a query of 2^31 letters or more");
  ChunkBuffers cb, up;
  upload_chunk(r, both_strands ? up : cb, qbytes, qoff, c);
  if (both_strands) {
    const uint64_t nbytes = up.h_off[nreads];
    cb.q.alloc(2 * nbytes + 16);
    cb.off.alloc(n + 1);
    cb.status.alloc(std::max<uint64_t>(n, 1));
    cb.h_off.resize(n + 1);
    for (uint64_t i = 0; i < nreads; i++) {
      cb.h_off[2 * i] = 2 * up.h_off[i];
      cb.h_off[2 * i + 1] = 2 * up.h_off[i] + (up.h_off[i + 1] - up.h_off[i]);
    }
    cb.h_off[n] = 2 * nbytes;
    cb.h_status.resize(n);
    launch_strand_expand(r, up.q.p, up.off.p, nreads, cb.q.p, cb.off.p, s);
  }
  DevBuf<uint64_t> na(n), aoff(n + 1), scratch(scan_tiles(n) + 1);
  launch_smems(r, cb.q.p, cb.off.p, n, min_len, na.p, nullptr, nullptr, cb.status.p, s);
  launch_scan(r, na.p, n, aoff.p, scratch.p, s);
  uint64_t total = 0;
  HIP_CHECK(hipMemcpyAsync(&total, aoff.p + n, 8, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipMemcpyAsync(cb.h_status.data(), cb.status.p, n, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
  if (both_strands) {
    for (uint64_t i = 0; i < n; i++)
      if (cb.h_status[i] != Q_OK) raise_bad_query(c.lo + i / 2, cb.h_status[i]);  // the read's own index
  } else {
    check_status(cb, c.lo);
  }
  if (total >= (1ull << 32)) throw ArgError("a chunk of queries with 2^32 SMEMs or more");
  DevBuf<uint64_t> soff(n + 1), d_gpos;
  DevBuf<Seed> seeds;
  uint64_t nhits = 0;
  if (total) {
    DevBuf<Anchor> d_smems(total);
    DevBuf<uint64_t> ranges(2 * total), located(total), hoff(total + 1), lscratch(scan_tiles(total) + 1);
    launch_smems(r, cb.q.p, cb.off.p, n, min_len, nullptr, aoff.p, d_smems.p, nullptr, s);
    launch_anchor_ranges(r, d_smems.p, total, max_hits, ranges.p, located.p, s);
    launch_scan(r, located.p, total, hoff.p, lscratch.p, s);
    HIP_CHECK(hipMemcpyAsync(&nhits, hoff.p + total, 8, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    if (nhits > anchor_hit_cap() && nreads > 1) return false;
    chain_launch(r, s, n + 1, chain_seed_off_kernel, aoff.p, hoff.p, n + 1, soff.p);
    if (nhits) {
      d_gpos.alloc(nhits);
      seeds.alloc(nhits);
      launch_locate(r, ranges.p, 2, hoff.p, total, nhits, d_gpos.p, nullptr, s);
      chain_launch(r, s, nhits, chain_expand_kernel, d_smems.p, hoff.p, total, d_gpos.p, nhits, seeds.p);
    }
    HIP_CHECK(hipStreamSynchronize(s));  // the records, ranges and offsets above are released here
  } else {
    HIP_CHECK(hipMemsetAsync(soff.p, 0, (n + 1) * 8, s));
  }
  DevBuf<uint64_t> nch(n), nmem(n), choff(n + 1), moff(n + 1);
  DevBuf<uint8_t> status(n);
  launch_chain(r, soff.p, seeds.p, n, P, nch.p, nmem.p, nullptr, nullptr, nullptr, nullptr, status.p, s);
  launch_scan(r, nch.p, n, choff.p, scratch.p, s);
  uint64_t nchains = 0, nmembers = 0;
  HIP_CHECK(hipMemcpyAsync(&nchains, choff.p + n, 8, hipMemcpyDeviceToHost, s));
  launch_scan(r, nmem.p, n, moff.p, scratch.p, s);  // `scratch` serves both scans: they are ordered on the stream
  HIP_CHECK(hipMemcpyAsync(&nmembers, moff.p + n, 8, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
  DevBuf<Chain> d_chains(std::max<uint64_t>(nchains, 1));
  DevBuf<Seed> d_members(std::max<uint64_t>(nmembers, 1));
  if (nchains) launch_chain(r, soff.p, seeds.p, n, P, nullptr, nullptr, choff.p, moff.p, d_chains.p, d_members.p, nullptr, s);
  if (sink) {
    (*sink)(r, ChainOnDevice{cb, c, nch.p, choff.p, moff.p, d_chains.p, d_members.p, nchains, nmembers, status.p});
    return true;
  }
  const size_t at_q = out.n_chains.size(), at_c = out.chains.size(), at_m = out.members.size();
  out.n_chains.resize(at_q + n);
  out.status.resize(at_q + n);
  out.chains.resize(at_c + nchains);
  HIP_CHECK(hipMemcpyAsync(out.n_chains.data() + at_q, nch.p, n * 8, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipMemcpyAsync(out.status.data() + at_q, status.p, n, hipMemcpyDeviceToHost, s));
  if (nchains) HIP_CHECK(hipMemcpyAsync(out.chains.data() + at_c, d_chains.p, nchains * sizeof(Chain), hipMemcpyDeviceToHost, s));
  if (want_members) {
    out.members.resize(at_m + nmembers);
    if (nmembers) HIP_CHECK(hipMemcpyAsync(out.members.data() + at_m, d_members.p, nmembers * sizeof(Seed), hipMemcpyDeviceToHost, s));
  }
  HIP_CHECK(hipStreamSynchronize(s));
  return true;
}

void chain_range(Replica& r, const uint8_t* qbytes, const uint64_t* qoff, Shard c, uint32_t min_len, uint64_t max_hits, const ChainParams& P,
                 bool want_members, ChainHits& out, const ChainSink* sink = nullptr, bool both_strands = false) {
  if (c.hi <= c.lo) return;
  if (chain_chunk(r, qbytes, qoff, c, min_len, max_hits, P, want_members, out, sink, both_strands)) return;
  const uint64_t mid = c.lo + (c.hi - c.lo) / 2;  // the capacity fallback: halves, in query order (between reads, never between a read's strands)
  chain_range(r, qbytes, qoff, Shard{c.lo, mid}, min_len, max_hits, P, want_members, out, sink, both_strands);
  chain_range(r, qbytes, qoff, Shard{mid, c.hi}, min_len, max_hits, P, want_members, out, sink, both_strands);
}

// awry_chain_batch: shards over the replicas, results stitched in query order into pinned-pool arrays.  The out-pointers are
// written only when everything has succeeded.
void chain_batch(awry_index* idx, const uint8_t* qbytes, const uint64_t* qoff, uint64_t n, uint32_t min_len, uint64_t max_hits, const ChainParams& P,
                 uint64_t** chain_off_out, awry_chain_t** chains_out, uint64_t** seed_off_out, awry_seed_t** seeds_out, uint8_t** status_out) {
  require_chain_index(idx->host.bwt_len);
  std::vector<ChainHits> res(std::max<size_t>(1, idx->reps.size()));
  for_each_replica(idx, n, [&](Replica& r, Shard sh, int g) {
    HIP_CHECK(hipSetDevice(r.device));
    for (Shard c : chunk_queries(qoff, sh.lo, sh.hi)) chain_range(r, qbytes, qoff, c, min_len, max_hits, P, seeds_out != nullptr, res[g]);
  });
  MBuf<uint64_t> choff, soff;
  MBuf<awry_chain_t> chains;
  MBuf<awry_seed_t> members;
  MBuf<uint8_t> st;
  choff.grow(n + 1);
  choff.p[0] = 0;
  if (status_out) st.grow(std::max<uint64_t>(1, n));
  uint64_t q = 0, total = 0, nmembers = 0;
  for (auto& x : res) {
    if (status_out && !x.status.empty()) memcpy(st.p + q, x.status.data(), x.status.size());
    for (uint64_t c : x.n_chains) { total += c; choff.p[++q] = total; }
    nmembers += x.members.size();
  }
  require(q == n, "internal: shard results do not cover the batch");
  if (chains_out) chains.grow(std::max<uint64_t>(1, total));
  if (seeds_out) { soff.grow(total + 1); members.grow(std::max<uint64_t>(1, nmembers)); }
  uint64_t at = 0, at_m = 0, run = 0;
  for (auto& x : res) {
    if (chains_out && !x.chains.empty()) pool_memcpy(chains.p + at, x.chains.data(), x.chains.size() * sizeof(awry_chain_t));
    if (seeds_out) {
      if (!x.members.empty()) pool_memcpy(members.p + at_m, x.members.data(), x.members.size() * sizeof(awry_seed_t));
      for (size_t j = 0; j < x.chains.size(); j++) { soff.p[at + j] = run; run += x.chains[j].n_seeds; }
      at_m += x.members.size();
    }
    at += x.chains.size();
  }
  require(at == total, "internal: shard results do not cover the chains");
  if (seeds_out) {
    require(run == nmembers, "internal: the chains' seed counts do not cover the members");
    soff.p[total] = run;
  }
  *chain_off_out = choff.release();
  if (chains_out) *chains_out = chains.release();
  if (seeds_out) { *seed_off_out = soff.release(); *seeds_out = members.release(); }
  if (status_out) *status_out = st.release();
}

}  // namespace
