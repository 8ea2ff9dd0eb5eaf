// chain_align_host.h -- the driver of awry_align_chains_batch: chain_chunk's flow through the chain fill pass (chain_host.h), then,
// with chains and members still on the device, the first chains of every query, the alignment count pass, a scan, the fill pass
// and the copy-out, in sub-batches
// A part of awry_hip.hip (one translation unit): included there, in order, after chain_host.h and edit_host.h, and not on its own.
#pragma once

namespace {

// ---- align chains (kernels_chain_align.hip.h) -----------------------------------------------------------------------------

static_assert(sizeof(Aln) == sizeof(awry_aln_t) && sizeof(awry_aln_t) == 24 && offsetof(Aln, t_end) == offsetof(awry_aln_t, t_end) &&
                  offsetof(Aln, edits) == offsetof(awry_aln_t, edits) && offsetof(Aln, status) == offsetof(awry_aln_t, status),
              "the kernels write awry_aln_t records");
static_assert(CHAIN_ALIGN_MAX_BAND == AWRY_CHAIN_ALIGN_MAX_BAND && CHAIN_ALIGN_MAX_SKEW == AWRY_CHAIN_ALIGN_MAX_SKEW &&
                  CHAIN_ALIGN_MAX_LEN == AWRY_CHAIN_ALIGN_MAX_LEN && ALN_OK == AWRY_ALN_OK && ALN_SKEW == AWRY_ALN_SKEW && ALN_BAD_CHAIN == AWRY_ALN_BAD_CHAIN,
              "the kernels' limits are the header's");

void require_chain_align_args(uint64_t max_alignments, uint32_t band) {
  if (max_alignments < 1) throw ArgError("max_alignments must be at least 1");
  if (band > (uint32_t)CHAIN_ALIGN_MAX_BAND) throw ArgError("band must be in 0..8 (AWRY_CHAIN_ALIGN_MAX_BAND)");
}

// Chains the alignment passes take per launch: their staging (records, run counts, offsets, and the class lists: 52 B per chain,
// plus the runs) is bounded by the sub-batch whatever the batch.  Read per call: AWRY_CHAIN_ALIGN_SUB_BATCH (tests shrink it).
uint64_t chain_align_sub_batch() {
  const char* e = getenv("AWRY_CHAIN_ALIGN_SUB_BATCH");
  const uint64_t v = e ? strtoull(e, nullptr, 10) : 0;
  return v ? std::min<uint64_t>(v, 1ull << 24) : (1ull << 18);
}

struct ChainAlnHits {  // one shard's result, in query order
  std::vector<uint64_t> n_alns;  // per query
  std::vector<uint8_t> status;   // per query: Q_OK or Q_SEED_CAP
  std::vector<awry_chain_t> chains;
  std::vector<awry_aln_t> alns;
  std::vector<uint64_t> n_ops;  // per alignment
  std::vector<uint32_t> cigar;  // the runs, back to back
};

// One chunk, from where chain_chunk's fill pass leaves it: the first min(n_chains, max_alignments) chains of every query (a count
// per query, a scan, their records and queries, a scan of their member counts, their members), then per sub-batch the count
// pass, the scan of the run counts and the fill pass, appended to `out`.
void align_chunk_chains(Replica& r, const uint8_t* text8, const ChainOnDevice& v, uint64_t max_alignments, int band, bool want_cigar, ChainAlnHits& out) {
  const hipStream_t s = r.stream;
  const uint64_t n = v.c.hi - v.c.lo;
  uint64_t Lmax = 1;
  for (uint64_t i = 0; i < n; i++) Lmax = std::max(Lmax, v.cb.h_off[i + 1] - v.cb.h_off[i]);
  DevBuf<uint64_t> taken(n), aoff(n + 1), scratch(scan_tiles(n) + 1);
  chain_launch(r, s, n, chain_align_take_kernel, v.n_chains, n, max_alignments, taken.p);
  launch_scan(r, taken.p, n, aoff.p, scratch.p, s);
  uint64_t total = 0;
  const size_t at_q = out.n_alns.size(), at_a = out.alns.size();
  out.n_alns.resize(at_q + n);
  out.status.resize(at_q + n);
  HIP_CHECK(hipMemcpyAsync(&total, aoff.p + n, 8, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipMemcpyAsync(out.n_alns.data() + at_q, taken.p, n * 8, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipMemcpyAsync(out.status.data() + at_q, v.status, n, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
  require(total <= v.nchains, "internal: more chains selected than the chunk has");
  if (!total) return;
  DevBuf<uint32_t> sel_query(total);
  DevBuf<Chain> sel_chains(total);
  DevBuf<uint64_t> mcnt(total), smoff(total + 1), sscratch(scan_tiles(total) + 1);
  chain_launch(r, s, n, chain_align_select_kernel, v.chain_off, v.chains, aoff.p, n, sel_query.p, sel_chains.p, mcnt.p);
  launch_scan(r, mcnt.p, total, smoff.p, sscratch.p, s);
  uint64_t nsel = 0;
  HIP_CHECK(hipMemcpyAsync(&nsel, smoff.p + total, 8, hipMemcpyDeviceToHost, s));
  out.chains.resize(at_a + total);
  out.alns.resize(at_a + total);
  out.n_ops.resize(at_a + total);
  HIP_CHECK(hipMemcpyAsync(out.chains.data() + at_a, sel_chains.p, total * sizeof(Chain), hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
  require(nsel <= v.nmembers, "internal: the selected chains have more members than the chunk");
  DevBuf<Seed> sel_members(std::max<uint64_t>(nsel, 1));
  chain_launch(r, s, n, chain_align_gather_kernel, v.member_off, v.members, aoff.p, smoff.p, n, sel_members.p);
  const uint64_t sub = std::min(chain_align_sub_batch(), total);
  DevBuf<Aln> alns(sub);
  DevBuf<uint64_t> nops(sub), coff(sub + 1), cscratch(scan_tiles(sub) + 1);
  for (uint64_t at = 0; at < total; at += sub) {
    const uint64_t c = std::min(sub, total - at);
    launch_chain_align(r, text8, v.cb.q.p, v.cb.off.p, sel_query.p + at, smoff.p + at, sel_members.p, c, band, (uint32_t)Lmax, alns.p, nops.p, nullptr, nullptr, s);
    uint64_t runs = 0;
    if (want_cigar) {
      launch_scan(r, nops.p, c, coff.p, cscratch.p, s);
      HIP_CHECK(hipMemcpyAsync(&runs, coff.p + c, 8, hipMemcpyDeviceToHost, s));
    }
    HIP_CHECK(hipMemcpyAsync(out.alns.data() + at_a + at, alns.p, c * sizeof(Aln), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(out.n_ops.data() + at_a + at, nops.p, c * 8, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    if (runs) {
      DevBuf<uint32_t> cigar(runs);
      launch_chain_align(r, text8, v.cb.q.p, v.cb.off.p, sel_query.p + at, smoff.p + at, sel_members.p, c, band, (uint32_t)Lmax, nullptr, nullptr, coff.p, cigar.p,
                         s);
      const size_t at_c = out.cigar.size();
      out.cigar.resize(at_c + runs);
      HIP_CHECK(hipMemcpyAsync(out.cigar.data() + at_c, cigar.p, runs * 4, hipMemcpyDeviceToHost, s));
      HIP_CHECK(hipStreamSynchronize(s));
    }
  }
}

// awry_align_chains_batch: shards over the replicas, results stitched in query order into pinned-pool arrays.  The out-pointers
// are written only when everything has succeeded.
void align_chains_batch(awry_index* idx, const uint8_t* qbytes, const uint64_t* qoff, uint64_t n, uint32_t min_len, uint64_t max_hits, const ChainParams& P,
                        uint64_t max_alignments, uint32_t band, uint64_t** aln_off_out, awry_chain_t** chains_out, awry_aln_t** alns_out,
                        uint64_t** cigar_off_out, uint32_t** cigar_out, uint8_t** status_out) {
  require_chain_index(idx->host.bwt_len);
  for (uint64_t i = 0; i < n; i++)
    if (qoff[i + 1] > qoff[i] && qoff[i + 1] - qoff[i] > (uint64_t)CHAIN_ALIGN_MAX_LEN)
      throw QueryError("query " + std::to_string(i) + ": longer than 1024 letters (AWRY_CHAIN_ALIGN_MAX_LEN)");
  const bool want_cigar = cigar_out != nullptr;
  std::vector<ChainAlnHits> res(std::max<size_t>(1, idx->reps.size()));
  for_each_replica(idx, n, [&](Replica& r, Shard sh, int g) {
    HIP_CHECK(hipSetDevice(r.device));
    const uint8_t* text8 = edit_text(r);
    const ChainSink sink = [&, g, text8](Replica& rr, const ChainOnDevice& v) { align_chunk_chains(rr, text8, v, max_alignments, (int)band, want_cigar, res[g]); };
    ChainHits unused;
    for (Shard c : chunk_queries(qoff, sh.lo, sh.hi)) chain_range(r, qbytes, qoff, c, min_len, max_hits, P, true, unused, &sink);
  });
  MBuf<uint64_t> aoff, coff;
  MBuf<awry_chain_t> chains;
  MBuf<awry_aln_t> alns;
  MBuf<uint32_t> cg;
  MBuf<uint8_t> st;
  aoff.grow(n + 1);
  aoff.p[0] = 0;
  if (status_out) st.grow(std::max<uint64_t>(1, n));
  uint64_t q = 0, total = 0, runs = 0;
  for (auto& x : res) {
    if (status_out && !x.status.empty()) memcpy(st.p + q, x.status.data(), x.status.size());
    for (uint64_t c : x.n_alns) { total += c; aoff.p[++q] = total; }
    runs += x.cigar.size();
  }
  require(q == n, "internal: shard results do not cover the batch");
  if (chains_out) chains.grow(std::max<uint64_t>(1, total));
  if (alns_out) alns.grow(std::max<uint64_t>(1, total));
  if (want_cigar) { coff.grow(total + 1); cg.grow(std::max<uint64_t>(1, runs)); }
  uint64_t at = 0, at_c = 0;
  for (auto& x : res) {
    require(x.chains.size() == x.alns.size() && x.alns.size() == x.n_ops.size(), "internal: the alignment passes do not cover the chains");
    if (chains_out && !x.chains.empty()) pool_memcpy(chains.p + at, x.chains.data(), x.chains.size() * sizeof(awry_chain_t));
    if (alns_out && !x.alns.empty()) pool_memcpy(alns.p + at, x.alns.data(), x.alns.size() * sizeof(awry_aln_t));
    if (want_cigar) {
      if (!x.cigar.empty()) pool_memcpy(cg.p + at_c, x.cigar.data(), x.cigar.size() * 4);
      for (size_t j = 0; j < x.n_ops.size(); j++) { coff.p[at + j] = at_c; at_c += x.n_ops[j]; }
    }
    at += x.alns.size();
  }
  require(at == total, "internal: shard results do not cover the alignments");
  if (want_cigar) {
    require(at_c == runs, "internal: the run counts do not cover the CIGAR runs");
    coff.p[total] = runs;
  }
  *aln_off_out = aoff.release();
  if (chains_out) *chains_out = chains.release();
  if (alns_out) *alns_out = alns.release();
  if (want_cigar) { *cigar_off_out = coff.release(); *cigar_out = cg.release(); }
  if (status_out) *status_out = st.release();
}

}  // namespace
