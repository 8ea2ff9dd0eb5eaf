// map_host.h -- the driver of awry_map_batch: chain_chunk's flow over the doubled batch (chain_host.h, both strands), then, with
// chains and members still on the device, the first chains of every query, the alignment count pass over all of them, the
// selection (count pass, scan, fill pass), the gather of the reported alignments, the CIGAR fill pass over those only, in
// sub-batches, and the copy-out
// A part of awry_hip.hip (one translation unit): included there, in order, after chain_align_host.h, and not on its own.
#pragma once

namespace {

// ---- map reads on both strands (kernels_map.hip.h) ----------------------------------------------------------------------------

static_assert(sizeof(MapRec) == sizeof(awry_map_t) && sizeof(awry_map_t) == 32 && offsetof(MapRec, t_end) == offsetof(awry_map_t, t_end) &&
                  offsetof(MapRec, edits) == offsetof(awry_map_t, edits) && offsetof(MapRec, chain_score) == offsetof(awry_map_t, chain_score) &&
                  offsetof(MapRec, chain_index) == offsetof(awry_map_t, chain_index) && offsetof(MapRec, strand) == offsetof(awry_map_t, strand) &&
                  offsetof(MapRec, mapq) == offsetof(awry_map_t, mapq) && offsetof(MapRec, flags) == offsetof(awry_map_t, flags),
              "the kernels write awry_map_t records");
static_assert(MAP_MAX_CHAINS == AWRY_MAP_MAX_CHAINS && MAP_SECONDARY == AWRY_MAP_SECONDARY && sizeof(awry_pos_t) == 16, "the kernels' limits are the header's");

void require_map_args(uint64_t chains_per_strand, uint64_t max_report, uint32_t band) {
  if (chains_per_strand < 1 || chains_per_strand > (uint64_t)MAP_MAX_CHAINS) throw ArgError("chains_per_strand must be in 1..8 (AWRY_MAP_MAX_CHAINS)");
  if (max_report < 1 || max_report > 2 * chains_per_strand) throw ArgError("max_report must be in 1 .. 2 * chains_per_strand");
  require_chain_align_args(1, band);
}

struct MapHits {  // one shard's result, in read order
  std::vector<uint64_t> n_maps;  // per read
  std::vector<uint8_t> status;   // per read: Q_OK or Q_SEED_CAP
  std::vector<awry_map_t> maps;
  std::vector<awry_pos_t> pos;
  std::vector<uint64_t> n_ops;  // per record
  std::vector<uint32_t> cigar;  // the runs, back to back
};

// One chunk, from where chain_chunk's fill pass leaves the doubled batch: the first min(n_chains, A) chains of each of the 2 n
// queries (align_chunk_chains' take / select / gather), the alignment count pass over all of them in sub-batches, the selection
// per read, and the CIGAR fill pass over the reported alignments, appended to `out`.
void map_chunk(Replica& r, const uint8_t* text8, const ChainOnDevice& v, uint32_t A, uint32_t R, int band, bool want_pos, bool want_cigar, MapHits& out) {
  const hipStream_t s = r.stream;
  const uint64_t n = v.c.hi - v.c.lo, n2 = 2 * n;
  uint64_t Lmax = 1;
  for (uint64_t i = 0; i < n2; i++) Lmax = std::max(Lmax, v.cb.h_off[i + 1] - v.cb.h_off[i]);
  DevBuf<uint64_t> taken(n2), aoff(n2 + 1), scratch(scan_tiles(n2) + 1);
  chain_launch(r, s, n2, chain_align_take_kernel, v.n_chains, n2, (uint64_t)A, taken.p);
  launch_scan(r, taken.p, n2, aoff.p, scratch.p, s);
  uint64_t total = 0;
  HIP_CHECK(hipMemcpyAsync(&total, aoff.p + n2, 8, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
  require(total <= v.nchains && total < (1ull << 32), "internal: more chains selected than the chunk has");
  const uint64_t tot1 = std::max<uint64_t>(total, 1);
  DevBuf<uint32_t> sel_query(tot1);
  DevBuf<Chain> sel_chains(tot1);
  DevBuf<uint64_t> smoff(total + 1), nops(tot1);
  DevBuf<Aln> alns(tot1);
  DevBuf<Seed> sel_members;
  if (total) {
    DevBuf<uint64_t> mcnt(total), sscratch(scan_tiles(total) + 1);
    chain_launch(r, s, n2, chain_align_select_kernel, v.chain_off, v.chains, aoff.p, n2, sel_query.p, sel_chains.p, mcnt.p);
    launch_scan(r, mcnt.p, total, smoff.p, sscratch.p, s);
    uint64_t nsel = 0;
    HIP_CHECK(hipMemcpyAsync(&nsel, smoff.p + total, 8, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    require(nsel <= v.nmembers, "internal: the selected chains have more members than the chunk");
    sel_members.alloc(std::max<uint64_t>(nsel, 1));
    chain_launch(r, s, n2, chain_align_gather_kernel, v.member_off, v.members, aoff.p, smoff.p, n2, sel_members.p);
    const uint64_t sub = std::min(chain_align_sub_batch(), total);
    for (uint64_t at = 0; at < total; at += sub)  // the count pass over every candidate: records and run counts stay on the device
      launch_chain_align(r, text8, v.cb.q.p, v.cb.off.p, sel_query.p + at, smoff.p + at, sel_members.p, std::min(sub, total - at), band, (uint32_t)Lmax,
                         alns.p + at, nops.p + at, nullptr, nullptr, s);
  }
  // the selection: records per read, a scan, the records
  DevBuf<uint64_t> nmaps(n), moff(n + 1);
  DevBuf<uint8_t> rstatus(n);
  launch_map_select(r, aoff.p, alns.p, sel_chains.p, v.status, n, A, R, nmaps.p, rstatus.p, nullptr, nullptr, nullptr, nullptr, s);
  launch_scan(r, nmaps.p, n, moff.p, scratch.p, s);
  uint64_t nwin = 0;
  const size_t at_q = out.n_maps.size(), at_m = out.maps.size();
  out.n_maps.resize(at_q + n);
  out.status.resize(at_q + n);
  HIP_CHECK(hipMemcpyAsync(&nwin, moff.p + n, 8, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipMemcpyAsync(out.n_maps.data() + at_q, nmaps.p, n * 8, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipMemcpyAsync(out.status.data() + at_q, rstatus.p, n, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
  require(nwin <= total, "internal: more records than candidates");
  if (!nwin) return;
  DevBuf<MapRec> maps(nwin);
  DevBuf<uint32_t> win(nwin);
  DevBuf<uint64_t> pos(want_pos ? 2 * nwin : 0);
  launch_map_select(r, aoff.p, alns.p, sel_chains.p, v.status, n, A, R, nullptr, nullptr, moff.p, maps.p, win.p, want_pos ? pos.p : nullptr, s);
  out.maps.resize(at_m + nwin);
  HIP_CHECK(hipMemcpyAsync(out.maps.data() + at_m, maps.p, nwin * sizeof(MapRec), hipMemcpyDeviceToHost, s));
  if (want_pos) {
    out.pos.resize(at_m + nwin);
    HIP_CHECK(hipMemcpyAsync(out.pos.data() + at_m, pos.p, nwin * sizeof(awry_pos_t), hipMemcpyDeviceToHost, s));
  }
  if (!want_cigar) {
    HIP_CHECK(hipStreamSynchronize(s));
    return;
  }
  // the reported alignments as a chain list of their own, then the fill pass over them only
  DevBuf<uint32_t> win_query(nwin);
  DevBuf<uint64_t> win_mcnt(nwin), win_nops(nwin), win_moff(nwin + 1), wscratch(scan_tiles(nwin) + 1);
  chain_launch(r, s, nwin, map_gather_kernel, win.p, nwin, sel_query.p, smoff.p, sel_members.p, nops.p, win_query.p, win_mcnt.p, win_nops.p, nullptr, nullptr);
  launch_scan(r, win_mcnt.p, nwin, win_moff.p, wscratch.p, s);
  uint64_t nwm = 0;
  out.n_ops.resize(at_m + nwin);
  HIP_CHECK(hipMemcpyAsync(&nwm, win_moff.p + nwin, 8, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipMemcpyAsync(out.n_ops.data() + at_m, win_nops.p, nwin * 8, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
  DevBuf<Seed> win_members(std::max<uint64_t>(nwm, 1));
  chain_launch(r, s, nwin, map_gather_kernel, win.p, nwin, sel_query.p, smoff.p, sel_members.p, nops.p, nullptr, nullptr, nullptr, win_moff.p, win_members.p);
  const uint64_t sub = std::min(chain_align_sub_batch(), nwin);
  DevBuf<uint64_t> coff(sub + 1), cscratch(scan_tiles(sub) + 1);
  for (uint64_t at = 0; at < nwin; at += sub) {
    const uint64_t c = std::min(sub, nwin - at);
    uint64_t runs = 0;
    launch_scan(r, win_nops.p + at, c, coff.p, cscratch.p, s);
    HIP_CHECK(hipMemcpyAsync(&runs, coff.p + c, 8, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    if (!runs) continue;
    DevBuf<uint32_t> cigar(runs);
    launch_chain_align(r, text8, v.cb.q.p, v.cb.off.p, win_query.p + at, win_moff.p + at, win_members.p, c, band, (uint32_t)Lmax, nullptr, nullptr, coff.p,
                       cigar.p, s);
    const size_t at_c = out.cigar.size();
    out.cigar.resize(at_c + runs);
    HIP_CHECK(hipMemcpyAsync(out.cigar.data() + at_c, cigar.p, runs * 4, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
  }
}

// awry_map_batch: shards over the replicas, results stitched in read order into pinned-pool arrays.  The out-pointers are written
// only when everything has succeeded.
void map_batch(awry_index* idx, const uint8_t* qbytes, const uint64_t* qoff, uint64_t n, uint32_t min_len, uint64_t max_hits, const ChainParams& P,
               uint32_t chains_per_strand, uint32_t max_report, uint32_t band, uint64_t** map_off_out, awry_map_t** maps_out, awry_pos_t** pos_out,
               uint64_t** cigar_off_out, uint32_t** cigar_out, uint8_t** status_out) {
  if (idx->host.alphabet != NUCLEOTIDE) throw ArgError("mapping on both strands needs a nucleotide index");
  require_chain_index(idx->host.bwt_len);
  for (uint64_t i = 0; i < n; i++)
    if (qoff[i + 1] > qoff[i] && qoff[i + 1] - qoff[i] > (uint64_t)CHAIN_ALIGN_MAX_LEN)
      throw QueryError("query " + std::to_string(i) + ": longer than 1024 letters (AWRY_CHAIN_ALIGN_MAX_LEN)");
  const bool want_cigar = cigar_out != nullptr, want_pos = pos_out != nullptr;
  std::vector<MapHits> res(std::max<size_t>(1, idx->reps.size()));
  for_each_replica(idx, n, [&](Replica& r, Shard sh, int g) {
    HIP_CHECK(hipSetDevice(r.device));
    const uint8_t* text8 = edit_text(r);
    const ChainSink sink = [&, g, text8](Replica& rr, const ChainOnDevice& v) {
      map_chunk(rr, text8, v, chains_per_strand, max_report, (int)band, want_pos, want_cigar, res[g]);
    };
    ChainHits unused;
    for (Shard c : chunk_queries(qoff, sh.lo, sh.hi, 2)) chain_range(r, qbytes, qoff, c, min_len, max_hits, P, true, unused, &sink, true);
  });
  MBuf<uint64_t> moff, coff;
  MBuf<awry_map_t> maps;
  MBuf<awry_pos_t> pos;
  MBuf<uint32_t> cg;
  MBuf<uint8_t> st;
  moff.grow(n + 1);
  moff.p[0] = 0;
  if (status_out) st.grow(std::max<uint64_t>(1, n));
  uint64_t q = 0, total = 0, runs = 0;
  for (auto& x : res) {
    if (status_out && !x.status.empty()) memcpy(st.p + q, x.status.data(), x.status.size());
    for (uint64_t c : x.n_maps) { total += c; moff.p[++q] = total; }
    runs += x.cigar.size();
  }
  require(q == n, "internal: shard results do not cover the batch");
  if (maps_out) maps.grow(std::max<uint64_t>(1, total));
  if (want_pos) pos.grow(std::max<uint64_t>(1, total));
  if (want_cigar) { coff.grow(total + 1); cg.grow(std::max<uint64_t>(1, runs)); }
  uint64_t at = 0, at_c = 0;
  for (auto& x : res) {
    require((!want_pos || x.pos.size() == x.maps.size()) && (!want_cigar || x.n_ops.size() == x.maps.size()), "internal: the passes do not cover the records");
    if (maps_out && !x.maps.empty()) pool_memcpy(maps.p + at, x.maps.data(), x.maps.size() * sizeof(awry_map_t));
    if (want_pos && !x.pos.empty()) pool_memcpy(pos.p + at, x.pos.data(), x.pos.size() * sizeof(awry_pos_t));
    if (want_cigar) {
      if (!x.cigar.empty()) pool_memcpy(cg.p + at_c, x.cigar.data(), x.cigar.size() * 4);
      for (size_t j = 0; j < x.n_ops.size(); j++) { coff.p[at + j] = at_c; at_c += x.n_ops[j]; }
    }
    at += x.maps.size();
  }
  require(at == total, "internal: shard results do not cover the records");
  if (want_cigar) {
    require(at_c == runs, "internal: the run counts do not cover the CIGAR runs");
    coff.p[total] = runs;
  }
  *map_off_out = moff.release();
  if (maps_out) *maps_out = maps.release();
  if (want_pos) *pos_out = pos.release();
  if (want_cigar) { *cigar_off_out = coff.release(); *cigar_out = cg.release(); }
  if (status_out) *status_out = st.release();
}

}  // namespace
