// chain_align_host.h -- the driver of awry_align_chains_batch, a sink of chain_chunk (chain_host.h): with chains and members still
// on the device, the first chains of every query (select_chains), then per sub-batch the alignment count pass, the CIGAR fill
// (fill_cigar) and the copy-out.  map_host.h uses the same two stages.
// A part of awry_hip.hip (one translation unit): included there, in order, after chain_host.h and edit_host.h, and not on its own.
#pragma once

namespace {

// ---- align chains (kernels_chain_align.hip.h) -----------------------------------------------------------------------------

static_assert(sizeof(Aln) == sizeof(awry_aln_t) && sizeof(awry_aln_t) == 24 && offsetof(Aln, t_end) == offsetof(awry_aln_t, t_end) &&
                  offsetof(Aln, edits) == offsetof(awry_aln_t, edits) && offsetof(Aln, status) == offsetof(awry_aln_t, status),
              "the kernels write awry_aln_t records");
static_assert(sizeof(AlnClip) == sizeof(awry_aln_clip_t) && sizeof(awry_aln_clip_t) == 32 && offsetof(AlnClip, t_end) == offsetof(awry_aln_clip_t, t_end) &&
                  offsetof(AlnClip, edits) == offsetof(awry_aln_clip_t, edits) && offsetof(AlnClip, status) == offsetof(awry_aln_clip_t, status) &&
                  offsetof(AlnClip, score) == offsetof(awry_aln_clip_t, score) && offsetof(AlnClip, clip_left) == offsetof(awry_aln_clip_t, clip_left) &&
                  offsetof(AlnClip, clip_right) == offsetof(awry_aln_clip_t, clip_right),
              "the kernels write awry_aln_clip_t records");
static_assert(CHAIN_ALIGN_MAX_BAND == AWRY_CHAIN_ALIGN_MAX_BAND && CHAIN_ALIGN_MAX_SKEW == AWRY_CHAIN_ALIGN_MAX_SKEW &&
                  CHAIN_ALIGN_MAX_LEN == AWRY_CHAIN_ALIGN_MAX_LEN && ALN_OK == AWRY_ALN_OK && ALN_SKEW == AWRY_ALN_SKEW && ALN_BAD_CHAIN == AWRY_ALN_BAD_CHAIN,
              "the kernels' limits are the header's");

void require_chain_align_args(uint64_t max_alignments, uint32_t band) {
  if (max_alignments < 1) throw ArgError("max_alignments must be at least 1");
  if (band > (uint32_t)CHAIN_ALIGN_MAX_BAND) throw ArgError("band must be in 0..8 (AWRY_CHAIN_ALIGN_MAX_BAND)");
}

// the clipped mode's weights (include/awry_hip.h, "soft-clip read ends"): match 1..16, mismatch and gap 0..64, end_bonus 0..1024
AlignMode clip_mode(uint32_t match, uint32_t mismatch, uint32_t gap, uint32_t end_bonus) {
  if (match < 1 || match > (uint32_t)AWRY_CLIP_MAX_MATCH) throw ArgError("match must be in 1..16 (AWRY_CLIP_MAX_MATCH)");
  if (mismatch > (uint32_t)AWRY_CLIP_MAX_PENALTY || gap > (uint32_t)AWRY_CLIP_MAX_PENALTY)
    throw ArgError("mismatch and gap must be in 0..64 (AWRY_CLIP_MAX_PENALTY)");
  if (end_bonus > (uint32_t)AWRY_CLIP_MAX_END_BONUS) throw ArgError("end_bonus must be in 0..1024 (AWRY_CLIP_MAX_END_BONUS)");
  return AlignMode{true, (int)match, (int)mismatch, (int)gap, (int)end_bonus};
}

// Chains the alignment passes take per launch: their staging (records, run counts, offsets, and the class lists: 52 B per chain,
// plus the runs) is bounded by the sub-batch whatever the batch.  Read per call: AWRY_CHAIN_ALIGN_SUB_BATCH (tests shrink it).
uint64_t chain_align_sub_batch() { return env_cap("AWRY_CHAIN_ALIGN_SUB_BATCH", 1ull << 18, 1ull << 24); }

template <class AlnT>  // awry_aln_t, or awry_aln_clip_t in the clipped mode
struct ChainAlnHitsOf {  // one shard's result, in query order
  std::vector<uint64_t> n_alns;  // per query
  std::vector<uint8_t> status;   // per query: Q_OK or Q_SEED_CAP
  std::vector<awry_chain_t> chains;
  std::vector<AlnT> alns;
  std::vector<uint64_t> n_ops;  // per alignment
  std::vector<uint32_t> cigar;  // the runs, back to back
};

template <class AlnT>  // the result arrays of the call: `off` always, the others where the caller wants them (the two cigar arrays together)
struct AlnOut { uint64_t** off; awry_chain_t** chains; AlnT** alns; uint64_t** cigar_off; uint32_t** cigar; uint8_t** status; };

// ---- the two stages shared with map_chunk (map_host.h) ----------------------------------------------------------------------------

struct SelectedChains {  // the first chains of every query, as a chain list of their own on the device
  DevBuf<uint64_t> taken, aoff, scratch;  // per query: chains taken, their offsets; the scratch of scans over the queries
  DevBuf<uint32_t> query;                 // per selected chain: its query
  DevBuf<Chain> chains;
  DevBuf<uint64_t> mcnt, moff, mscratch;  // per selected chain: members, their offsets
  DevBuf<Seed> members;
  uint64_t total = 0, nsel = 0;           // selected chains, and their members
  void release_scratch() { mcnt.reset(); mscratch.reset(); }
};

// The first min(n_chains, take) chains of each of v's nq queries: a count per query, a scan, their records and queries, a scan of
// their member counts, their members.  Two stream synchronisations; without a chain only the first, and only `taken`, `aoff` and
// `scratch` are allocated.  Returns with the gather queued.
void select_chains(Replica& r, const ChainOnDevice& v, uint64_t nq, uint64_t take, SelectedChains& S) {
  const hipStream_t s = r.stream;
  S.taken.alloc(nq); S.aoff.alloc(nq + 1); S.scratch.alloc(scan_tiles(nq) + 1);
  flat_launch(r, s, nq, chain_align_take_kernel, v.n_chains, nq, take, S.taken.p);
  scan_with_total(r, S.taken.p, nq, S.aoff.p, S.scratch.p, &S.total, s);
  HIP_CHECK(hipStreamSynchronize(s));
  const uint64_t total = S.total;
  require(total <= v.nchains && total < (1ull << 32), "internal: more chains selected than the chunk has");
  if (!total) return;
  S.query.alloc(total); S.chains.alloc(total); S.mcnt.alloc(total); S.moff.alloc(total + 1); S.mscratch.alloc(scan_tiles(total) + 1);
  flat_launch(r, s, nq, chain_align_select_kernel, v.chain_off, v.chains, S.aoff.p, nq, S.query.p, S.chains.p, S.mcnt.p);
  scan_with_total(r, S.mcnt.p, total, S.moff.p, S.mscratch.p, &S.nsel, s);
  HIP_CHECK(hipStreamSynchronize(s));
  require(S.nsel <= v.nmembers, "internal: the selected chains have more members than the chunk");
  S.members.alloc(std::max<uint64_t>(S.nsel, 1));
  flat_launch(r, s, nq, chain_align_gather_kernel, v.member_off, v.members, S.aoff.p, S.moff.p, nq, S.members.p);
}

// The CIGAR fill of one sub-batch: c chains (their queries, member offsets and members as launch_chain_align takes them) whose run
// counts lie in d_nops.  Scan of the run counts, the runs read back, and if there are any the fill pass and its runs appended to
// `cigar`.  d_coff (c + 1) and d_cscratch (scan_tiles(c) + 1) are the caller's.  Two stream synchronisations, without runs one:
// what the caller has queued before rides on the first.
void fill_cigar(Replica& r, const uint8_t* text8, const ChunkBuffers& cb, const uint32_t* d_query, const uint64_t* d_moff, const Seed* d_members, uint64_t c,
                int band, const AlignMode& md, uint32_t Lmax, const uint64_t* d_nops, uint64_t* d_coff, uint64_t* d_cscratch, std::vector<uint32_t>& cigar) {
  const hipStream_t s = r.stream;
  uint64_t runs = 0;
  scan_with_total(r, d_nops, c, d_coff, d_cscratch, &runs, s);
  HIP_CHECK(hipStreamSynchronize(s));
  if (!runs) return;
  DevBuf<uint32_t> d_cigar(runs);
  launch_chain_align(r, text8, cb.q.p, cb.off.p, d_query, d_moff, d_members, c, band, md, Lmax, nullptr, nullptr, d_coff, d_cigar.p, s);
  const size_t at_c = cigar.size();
  cigar.resize(at_c + runs);
  HIP_CHECK(hipMemcpyAsync(cigar.data() + at_c, d_cigar.p, runs * 4, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
}

// One chunk, from where chain_chunk's fill pass leaves it: the first min(n_chains, max_alignments) chains of every query, then
// per sub-batch the count pass and the CIGAR fill, so that the staging is bounded by the sub-batch; appended to `out`.  AlnT is the
// record of md's mode.
template <class AlnT>
void align_chunk_chains(Replica& r, const uint8_t* text8, const ChainOnDevice& v, uint64_t max_alignments, int band, const AlignMode& md, bool want_cigar,
                        ChainAlnHitsOf<AlnT>& out) {
  static_assert(sizeof(AlnT) == sizeof(AlnOf<std::is_same_v<AlnT, awry_aln_clip_t>>), "the record of the mode");
  require(md.clip == std::is_same_v<AlnT, awry_aln_clip_t>, "internal: the alignment records are not the mode's");
  const hipStream_t s = r.stream;
  const uint64_t n = v.c.hi - v.c.lo;
  uint64_t Lmax = 1;
  for (uint64_t i = 0; i < n; i++) Lmax = std::max(Lmax, v.cb.h_off[i + 1] - v.cb.h_off[i]);
  const size_t at_q = out.n_alns.size(), at_a = out.alns.size();
  out.n_alns.resize(at_q + n);  // (zeros: what a chunk without a chain reports)
  out.status.resize(at_q + n);
  HIP_CHECK(hipMemcpyAsync(out.status.data() + at_q, v.status, n, hipMemcpyDeviceToHost, s));  // rides on the selection's first wait
  SelectedChains S;
  select_chains(r, v, n, max_alignments, S);
  const uint64_t total = S.total;
  if (!total) return;
  out.chains.resize(at_a + total);
  out.alns.resize(at_a + total);
  out.n_ops.resize(at_a + total);
  // these two ride on the first sub-batch's wait
  HIP_CHECK(hipMemcpyAsync(out.n_alns.data() + at_q, S.taken.p, n * 8, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipMemcpyAsync(out.chains.data() + at_a, S.chains.p, total * sizeof(Chain), hipMemcpyDeviceToHost, s));
  const uint64_t sub = std::min(chain_align_sub_batch(), total);
  DevBuf<AlnT> alns(sub);
  DevBuf<uint64_t> nops(sub), coff(sub + 1), cscratch(scan_tiles(sub) + 1);
  for (uint64_t at = 0; at < total; at += sub) {
    const uint64_t c = std::min(sub, total - at);
    launch_chain_align(r, text8, v.cb.q.p, v.cb.off.p, S.query.p + at, S.moff.p + at, S.members.p, c, band, md, (uint32_t)Lmax, alns.p, nops.p, nullptr, nullptr,
                       s);
    HIP_CHECK(hipMemcpyAsync(out.alns.data() + at_a + at, alns.p, c * sizeof(AlnT), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(out.n_ops.data() + at_a + at, nops.p, c * 8, hipMemcpyDeviceToHost, s));
    if (want_cigar) fill_cigar(r, text8, v.cb, S.query.p + at, S.moff.p + at, S.members.p, c, band, md, (uint32_t)Lmax, nops.p, coff.p, cscratch.p,
                               out.cigar);
    else HIP_CHECK(hipStreamSynchronize(s));
  }
}

// awry_align_chains_batch: shards over the replicas, results stitched in query order into pinned-pool arrays.  The out-pointers
// are written only when everything has succeeded.  awry_align_chains_clip_batch is the same with md's mode and AlnT = awry_aln_clip_t.
template <class AlnT>
void align_chains_batch(awry_index* idx, const Reads& q, const Seeding& sc, uint64_t max_alignments, uint32_t band, const AlignMode& md, const AlnOut<AlnT>& out) {
  require_chain_index(idx->host.bwt_len);
  require_chain_align_lengths(q.off, q.n);
  const bool want_cigar = out.cigar != nullptr;
  using Hits = ChainAlnHitsOf<AlnT>;
  std::vector<Hits> res(std::max<size_t>(1, idx->reps.size()));
  for_each_replica(idx, q.n, [&](Replica& r, Shard sh, int g) {
    HIP_CHECK(hipSetDevice(r.device));
    const uint8_t* text8 = edit_text(r);
    const auto sink = [&, g, text8](Replica& rr, const ChainOnDevice& v) { align_chunk_chains(rr, text8, v, max_alignments, (int)band, md, want_cigar, res[g]); };
    for (Shard c : chunk_queries(q.off, sh.lo, sh.hi))
      halve_until_fits(c, [&](Shard h) { return chain_chunk(r, q, h, sc, false, sink); });
  });
  MBuf<uint64_t> aoff, coff;
  MBuf<awry_chain_t> chains;
  MBuf<AlnT> alns;
  MBuf<uint32_t> cg;
  MBuf<uint8_t> st;
  const uint64_t total = stitch_offsets(res, &Hits::n_alns, q.n, aoff);
  for (auto& x : res) require(x.chains.size() == x.alns.size() && x.alns.size() == x.n_ops.size(), "internal: the alignment passes do not cover the chains");
  require(stitch_size(res, &Hits::alns) == total, "internal: shard results do not cover the alignments");
  if (out.status) stitch_concat(res, &Hits::status, st);
  if (out.chains) stitch_concat(res, &Hits::chains, chains);
  if (out.alns) stitch_concat(res, &Hits::alns, alns);
  if (want_cigar) stitch_run_offsets(res, &Hits::n_ops, total, stitch_concat(res, &Hits::cigar, cg), coff);
  *out.off = aoff.release();
  if (out.chains) *out.chains = chains.release();
  if (out.alns) *out.alns = alns.release();
  if (want_cigar) { *out.cigar_off = coff.release(); *out.cigar = cg.release(); }
  if (out.status) *out.status = st.release();
}

}  // namespace
