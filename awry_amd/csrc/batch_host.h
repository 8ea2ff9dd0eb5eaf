// batch_host.h -- what the batch drivers of the read pipelines share (mismatch_host.h, anchor_host.h, chain_host.h, edit_host.h,
// chain_align_host.h, map_host.h, split_host.h, pair_host.h): the reads of a call and their two checks, the reader of the capacity
// variables, the flat launch, the scan that reads its total back, the chunk upload, the halving fallback and the stitching of the
// shards' results into the pinned result arrays.  Plain functions and structs: each driver still reads top to bottom in its own file.
// A part of awry_hip.hip (one translation unit): included there, in order, before the drivers, and not on its own.
#pragma once

namespace {

struct Reads { const uint8_t* bytes; const uint64_t* off; uint64_t n; };  // of a batch call: read i is bytes[off[i] .. off[i + 1])

// the first two checks of the entry points; first_out is the result array a call always writes (its offsets)
Reads checked_reads(const void* idx, const uint8_t* qbytes, const uint64_t* qoff, uint64_t n, const void* first_out) {
  require(idx && qoff && first_out, "null argument");
  require(qbytes || qoff[n] == qoff[0], "null query bytes");
  return Reads{qbytes, qoff, n};
}

void require_cigar_pair(const void* cigar_off_out, const void* cigar_out) {
  require((cigar_off_out == nullptr) == (cigar_out == nullptr), "cigar_off_out and cigar_out are given or omitted together");
}

// A capacity a test may shrink: the value of the environment variable `name` up to `max`, `dflt` when it is unset or 0.  Read per call.
uint64_t env_cap(const char* name, uint64_t dflt, uint64_t max) {
  const char* e = getenv(name);
  const uint64_t v = e ? strtoull(e, nullptr, 10) : 0;
  return v ? std::min(v, max) : dflt;
}

// one thread per item, blocks of 256
template <class K, class... Args>
void flat_launch(Replica& r, hipStream_t s, uint64_t items, K kernel, Args... args) {
  hipLaunchKernelGGL(kernel, dim3(grid_for(r, items, 256)), dim3(256), 0, s, args...);
  HIP_CHECK(hipGetLastError());
}

// The scan of a two-pass stage (count pass, scan, fill pass) and the copy of its total, d_off[n], into *total, both queued on s: the
// caller places the wait, so that what it queues before it rides on it.
void scan_with_total(Replica& r, const uint64_t* d_counts, uint64_t n, uint64_t* d_off, uint64_t* d_scratch, uint64_t* total, hipStream_t s) {
  launch_scan(r, d_counts, n, d_off, d_scratch, s);
  HIP_CHECK(hipMemcpyAsync(total, d_off + n, 8, hipMemcpyDeviceToHost, s));
}

// upload one chunk's query bytes and chunk-relative offsets (the generic count path's layout)
void upload_chunk(Replica& r, ChunkBuffers& cb, const uint8_t* qbytes, const uint64_t* qoff, Shard c) {
  const uint64_t n = c.hi - c.lo, base = qoff[c.lo], nbytes = qoff[c.hi] - base;
  cb.h_off.resize(n + 1);
  for (uint64_t i = 0; i <= n; i++) {
    if (qoff[c.lo + i] < base || (i && qoff[c.lo + i] < qoff[c.lo + i - 1])) throw ArgError("query offsets must be non-decreasing");
    cb.h_off[i] = qoff[c.lo + i] - base;
  }
  if (cb.q.n < nbytes + 16) cb.q.alloc(nbytes + 16);
  if (cb.off.n < n + 1) cb.off.alloc(n + 1);
  if (cb.status.n < n) cb.status.alloc(n);
  if (nbytes) HIP_CHECK(hipMemcpyAsync(cb.q.p, qbytes + base, nbytes, hipMemcpyHostToDevice, r.stream));
  HIP_CHECK(hipMemcpyAsync(cb.off.p, cb.h_off.data(), (n + 1) * 8, hipMemcpyHostToDevice, r.stream));
  cb.h_status.resize(n);
}

// the alignment kernels of kernels_chain_align.hip.h take queries of up to CHAIN_ALIGN_MAX_LEN letters
void require_chain_align_lengths(const uint64_t* qoff, uint64_t n) {
  for (uint64_t i = 0; i < n; i++)
    if (qoff[i + 1] > qoff[i] && qoff[i + 1] - qoff[i] > (uint64_t)CHAIN_ALIGN_MAX_LEN)
      throw QueryError("query " + std::to_string(i) + ": longer than 1024 letters (AWRY_CHAIN_ALIGN_MAX_LEN)");
}

// The capacity fallback of every chunk driver: chunk(Shard) returns false for "over capacity, nothing appended" (never for a
// shard of one query); the shard is then split in halves and each half redone, in query order.
template <class Chunk>
void halve_until_fits(Shard c, Chunk&& chunk) {
  if (c.hi <= c.lo || chunk(c)) return;
  const uint64_t mid = c.lo + (c.hi - c.lo) / 2;
  halve_until_fits(Shard{c.lo, mid}, chunk);
  halve_until_fits(Shard{mid, c.hi}, chunk);
}

// ---- stitching: shards are contiguous in query order, so every result array is the concatenation of theirs --------------------
// `res` holds one result struct per shard, `m` names one of its vectors.  The arrays are MBufs, which the batch function releases
// into its out-pointers only after everything has succeeded.

// counts per query -> the batch's CSR offsets; -> their total
template <class R>
uint64_t stitch_offsets(const std::vector<R>& res, std::vector<uint64_t> R::*m, uint64_t n, MBuf<uint64_t>& off) {
  off.grow(n + 1);
  off.p[0] = 0;
  uint64_t q = 0, total = 0;
  for (auto& x : res)
    for (uint64_t c : x.*m) {
      require(q < n, "internal: shard results do not cover the batch");
      total += c;
      off.p[++q] = total;
    }
  require(q == n, "internal: shard results do not cover the batch");
  return total;
}

template <class R, class T>
uint64_t stitch_size(const std::vector<R>& res, std::vector<T> R::*m) {
  uint64_t total = 0;
  for (auto& x : res) total += (x.*m).size();
  return total;
}

// one vector of every shard, back to back (at least one element is allocated: the caller frees a non-null array); -> the elements
template <class R, class T>
uint64_t stitch_concat(const std::vector<R>& res, std::vector<T> R::*m, MBuf<T>& out) {
  out.grow(std::max<uint64_t>(1, stitch_size(res, m)));
  uint64_t at = 0;
  for (auto& x : res) {
    const std::vector<T>& v = x.*m;
    if (!v.empty()) pool_memcpy(out.p + at, v.data(), v.size() * sizeof(T));
    at += v.size();
  }
  return at;
}

// run counts per record -> the run offsets of the `total` records, whose `runs` CIGAR runs lie back to back
template <class R, class T>
void stitch_run_offsets(const std::vector<R>& res, std::vector<T> R::*m, uint64_t total, uint64_t runs, MBuf<uint64_t>& coff) {
  require(stitch_size(res, m) == total, "internal: the run counts do not cover the records");
  coff.grow(total + 1);
  uint64_t at = 0, at_c = 0;
  for (auto& x : res)
    for (T c : x.*m) { coff.p[at++] = at_c; at_c += c; }
  require(at_c == runs, "internal: the run counts do not cover the CIGAR runs");
  coff.p[total] = runs;
}

}  // namespace
