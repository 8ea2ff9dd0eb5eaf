// chain_host.h -- the chunk driver of chaining: the record-locate stage of anchor_host.h over SMEMs, then seeds, the chain count
// pass, two scans and the fill pass, whose chains and members go to a sink on the device: awry_chain_batch's copy-out here, the
// alignment drivers of chain_align_host.h and map_host.h
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

struct Seeding {  // the seeding and chaining parameters of a call, checked in the order the entry points report them
  uint32_t min_len; uint64_t max_hits; ChainParams P;
  Seeding(uint32_t min_len, uint64_t max_hits, uint32_t max_seeds, uint32_t lookback, uint32_t max_gap, uint32_t max_skew, uint32_t min_score)
      : min_len(min_len), max_hits(max_hits) {
    require_smem_args(min_len);
    require(max_hits != 0, "max_hits must be at least 1 (a one-letter match has a quarter of the text as hits)");
    P = chain_params(max_seeds, lookback, max_gap, max_skew, min_score);
  }
};

void require_chain_index(uint64_t bwt_len) {
  if (bwt_len >= (1ull << 32)) throw ArgError("chaining needs an index with bwt_len < 2^32");
}

struct ChainHits {  // one shard's result, in query order
  std::vector<uint64_t> n_chains;  // per query
  std::vector<uint8_t> status;     // per query: Q_OK or Q_SEED_CAP
  std::vector<awry_chain_t> chains;
  std::vector<awry_seed_t> members;
};

// what a chunk's fill pass leaves on the device, for its sink
struct ChainOnDevice {
  const ChunkBuffers& cb;  // the chunk's queries
  Shard c;                 // the chunk's reads (with both strands, two queries each)
  const uint64_t *n_chains, *chain_off, *member_off;  // per query
  const Chain* chains;
  const Seed* members;
  uint64_t nchains, nmembers;
  const uint8_t* status;  // per query: Q_OK or Q_SEED_CAP
};

// The record-locate stage over SMEMs (text positions only); then one seed per located hit, the chain count pass, the scans of
// chains and members, the fill pass, and sink(r, ChainOnDevice), which returns with the stream synchronised.  false: the chunk's
// located hits exceed the capacity and it holds more than one read -- the sink has not been called.  both_strands: every read is
// two queries, itself and its reverse complement (find_records, copies == 2); the sink's view is over the 2 (c.hi - c.lo) queries.
// unit: find_records' (2 for read pairs, whose chunks are cut between pairs).
template <class Sink>
bool chain_chunk(Replica& r, const Reads& q, Shard c, const Seeding& sc, bool both_strands, Sink&& sink, uint64_t unit = 1) {
  const hipStream_t s = r.stream;
  const uint64_t n = (both_strands ? 2 : 1) * (c.hi - c.lo);
  for (uint64_t i = c.lo; i < c.hi; i++)
    if (q.off[i + 1] >= q.off[i] && q.off[i + 1] - q.off[i] >= (1ull << 31)) throw ArgError("a query of 2^31 letters or more");
  LocatedRecords L;
  if (!find_records(r, q.bytes, q.off, c, smem_finder(sc.min_len), sc.max_hits, both_strands ? 2 : 1, "SMEMs", L, unit)) return false;
  DevBuf<uint64_t> soff(n + 1);
  DevBuf<Seed> seeds;
  if (L.total) {
    flat_launch(r, s, n + 1, chain_seed_off_kernel, L.rec_off.p, L.hit_off.p, n + 1, soff.p);
    if (L.nhits) {
      seeds.alloc(L.nhits);
      locate_records(r, L, false);
      flat_launch(r, s, L.nhits, chain_expand_kernel, L.rec.p, L.hit_off.p, L.total, L.gpos.p, L.nhits, seeds.p);
    }
    HIP_CHECK(hipStreamSynchronize(s));
    L.release_records();  // records, ranges, located counts, their offsets and scratch: gone before the chain passes allocate
  } else {
    HIP_CHECK(hipMemsetAsync(soff.p, 0, (n + 1) * 8, s));
  }
  DevBuf<uint64_t> nch(n), nmem(n), choff(n + 1), moff(n + 1);
  DevBuf<uint8_t> status(n);
  launch_chain(r, soff.p, seeds.p, n, sc.P, nch.p, nmem.p, nullptr, nullptr, nullptr, nullptr, status.p, s);
  uint64_t nchains = 0, nmembers = 0;
  scan_with_total(r, nch.p, n, choff.p, L.scratch.p, &nchains, s);
  scan_with_total(r, nmem.p, n, moff.p, L.scratch.p, &nmembers, s);  // the stage's scratch serves both scans: they are ordered on the stream
  HIP_CHECK(hipStreamSynchronize(s));
  DevBuf<Chain> d_chains(std::max<uint64_t>(nchains, 1));
  DevBuf<Seed> d_members(std::max<uint64_t>(nmembers, 1));
  if (nchains) launch_chain(r, soff.p, seeds.p, n, sc.P, nullptr, nullptr, choff.p, moff.p, d_chains.p, d_members.p, nullptr, s);
  sink(r, ChainOnDevice{L.cb, c, nch.p, choff.p, moff.p, d_chains.p, d_members.p, nchains, nmembers, status.p});
  return true;
}

// awry_chain_batch's sink: the copy-out
void copy_out_chains(Replica& r, const ChainOnDevice& v, bool want_members, ChainHits& out) {
  const hipStream_t s = r.stream;
  const uint64_t n = v.c.hi - v.c.lo, nchains = v.nchains, nmembers = v.nmembers;
  const size_t at_q = out.n_chains.size(), at_c = out.chains.size(), at_m = out.members.size();
  out.n_chains.resize(at_q + n);
  out.status.resize(at_q + n);
  out.chains.resize(at_c + nchains);
  HIP_CHECK(hipMemcpyAsync(out.n_chains.data() + at_q, v.n_chains, n * 8, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipMemcpyAsync(out.status.data() + at_q, v.status, n, hipMemcpyDeviceToHost, s));
  if (nchains) HIP_CHECK(hipMemcpyAsync(out.chains.data() + at_c, v.chains, nchains * sizeof(Chain), hipMemcpyDeviceToHost, s));
  if (want_members) {
    out.members.resize(at_m + nmembers);
    if (nmembers) HIP_CHECK(hipMemcpyAsync(out.members.data() + at_m, v.members, nmembers * sizeof(Seed), hipMemcpyDeviceToHost, s));
  }
  HIP_CHECK(hipStreamSynchronize(s));
}

// awry_chain_batch: shards over the replicas, results stitched in query order into pinned-pool arrays.  The out-pointers are
// written only when everything has succeeded.
void chain_batch(awry_index* idx, const Reads& q, const Seeding& sc, uint64_t** chain_off_out, awry_chain_t** chains_out, uint64_t** seed_off_out,
                 awry_seed_t** seeds_out, uint8_t** status_out) {
  require_chain_index(idx->host.bwt_len);
  std::vector<ChainHits> res(std::max<size_t>(1, idx->reps.size()));
  for_each_replica(idx, q.n, [&](Replica& r, Shard sh, int g) {
    HIP_CHECK(hipSetDevice(r.device));
    const auto sink = [&, g](Replica& rr, const ChainOnDevice& v) { copy_out_chains(rr, v, seeds_out != nullptr, res[g]); };
    for (Shard c : chunk_queries(q.off, sh.lo, sh.hi))
      halve_until_fits(c, [&](Shard h) { return chain_chunk(r, q, h, sc, false, sink); });
  });
  MBuf<uint64_t> choff, soff;
  MBuf<awry_chain_t> chains;
  MBuf<awry_seed_t> members;
  MBuf<uint8_t> st;
  const uint64_t total = stitch_offsets(res, &ChainHits::n_chains, q.n, choff);
  require(stitch_size(res, &ChainHits::chains) == total, "internal: shard results do not cover the chains");
  if (status_out) stitch_concat(res, &ChainHits::status, st);
  if (chains_out) stitch_concat(res, &ChainHits::chains, chains);
  if (seeds_out) {  // the members, and per chain the offset of its first: the chains' seed counts, summed
    const uint64_t nmembers = stitch_concat(res, &ChainHits::members, members);
    soff.grow(total + 1);
    uint64_t at = 0, run = 0;
    for (auto& x : res)
      for (const awry_chain_t& ch : x.chains) { soff.p[at++] = run; run += ch.n_seeds; }
    require(run == nmembers, "internal: the chains' seed counts do not cover the members");
    soff.p[total] = run;
  }
  *chain_off_out = choff.release();
  if (chains_out) *chains_out = chains.release();
  if (seeds_out) { *seed_off_out = soff.release(); *seeds_out = members.release(); }
  if (status_out) *status_out = st.release();
}

}  // namespace
