// kernels_scan.hip.h -- wave / block scans, the exclusive scan of u64 counts, and small glue kernels.
// A part of kernels.hip.h (one header, cut by kernel family): included there, in order, and not on its own.
#pragma once

namespace awry {

// ------------------------------------------------------------------------------------------------
// exclusive scan of u64 counts (locate's CSR offsets): per-tile sums, scan of tile sums, fix-up
// ------------------------------------------------------------------------------------------------
constexpr int SCAN_TILE = 2048;  // elements per 256-thread block

__device__ __forceinline__ uint64_t wave_incl_scan(uint64_t v) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    uint64_t o = __shfl_up(v, d, 64);
    if (lane >= d) v += o;
  }
  return v;
}

// block-wide exclusive scan of one value per thread (256 threads); returns exclusive prefix, total in *tot
__device__ __forceinline__ uint64_t block_excl_scan(uint64_t v, uint64_t* tot) {
  __shared__ uint64_t wsum[4];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  uint64_t inc = wave_incl_scan(v);
  if (lane == 63) wsum[wv] = inc;
  __syncthreads();
  uint64_t base = 0, t = 0;
#pragma unroll
  for (int i = 0; i < 4; i++) {
    if (i < wv) base += wsum[i];
    t += wsum[i];
  }
  __syncthreads();
  *tot = t;
  return base + inc - v;
}

__global__ __launch_bounds__(256) void scan_tile_sums_kernel(const uint64_t* __restrict__ in, uint64_t n,
                                                             uint64_t* __restrict__ tile_sums) {
  const uint64_t base = (uint64_t)blockIdx.x * SCAN_TILE;
  uint64_t s = 0;
  for (int j = 0; j < SCAN_TILE / 256; j++) {
    uint64_t i = base + (uint64_t)j * 256 + threadIdx.x;
    if (i < n) s += in[i];
  }
  uint64_t tot;
  block_excl_scan(s, &tot);
  if (threadIdx.x == 0) tile_sums[blockIdx.x] = tot;
}

// single block: exclusive scan of tile sums in place; writes the grand total to *total
__global__ __launch_bounds__(256) void scan_tile_offsets_kernel(uint64_t* __restrict__ tile_sums, uint64_t ntiles,
                                                                uint64_t* __restrict__ total) {
  uint64_t carry = 0;
  for (uint64_t b = 0; b < ntiles; b += 256) {
    uint64_t i = b + threadIdx.x;
    uint64_t v = i < ntiles ? tile_sums[i] : 0, tot;
    uint64_t ex = block_excl_scan(v, &tot);
    if (i < ntiles) tile_sums[i] = carry + ex;
    carry += tot;
  }
  if (threadIdx.x == 0) *total = carry;
}

// out has n + 1 entries; out[n] = grand total
__global__ __launch_bounds__(256) void scan_apply_kernel(const uint64_t* __restrict__ in, uint64_t n,
                                                         const uint64_t* __restrict__ tile_offs,
                                                         uint64_t* __restrict__ out) {
  const uint64_t base = (uint64_t)blockIdx.x * SCAN_TILE;
  uint64_t carry = tile_offs[blockIdx.x];
  for (int j = 0; j < SCAN_TILE / 256; j++) {
    uint64_t i = base + (uint64_t)j * 256 + threadIdx.x;
    uint64_t v = i < n ? in[i] : 0, tot;
    uint64_t ex = block_excl_scan(v, &tot);
    if (i < n) out[i] = carry + ex;
    if (i == n - 1) out[n] = carry + ex + v;
    carry += tot;
  }
}

// measurement aid: device-to-device copy, 16 bytes per lane per step (the streaming rate the roofline object prints next to
// the nominal HBM peak)
__global__ __launch_bounds__(256) void stream_copy_kernel(const uint4* __restrict__ src, uint4* __restrict__ dst, uint64_t n16) {
  typedef unsigned int v4u __attribute__((ext_vector_type(4)));
  const v4u* __restrict__ s4 = reinterpret_cast<const v4u*>(src);
  v4u* __restrict__ d4 = reinterpret_cast<v4u*>(dst);
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n16; i += stride)
    __builtin_nontemporal_store(__builtin_nontemporal_load(&s4[i]), &d4[i]);
}

// profiling aid: an empty kernel whose grid size names a phase of a benchmark run, so that the per-dispatch rows of a
// rocprofv3 counter pass (which cannot be combined with marker tracing on this pool) can be cut into those phases
__global__ void phase_marker_kernel() {}

// counts as 32-bit words for the trip over PCIe (host-packed paths: a count is < bwt_len < 2^32 there)
__global__ __launch_bounds__(256) void narrow_counts_kernel(const uint64_t* __restrict__ in, uint32_t* __restrict__ out, uint64_t n) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) out[i] = (uint32_t)in[i];
}

// the lowest query of a chunk that the generic kernel rejected, as (index << 8 | status), or ~0: eight bytes cross PCIe
// instead of one status byte per query
__global__ __launch_bounds__(256) void status_first_bad_kernel(const uint8_t* __restrict__ status, uint64_t n, unsigned long long* __restrict__ first_bad) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  unsigned long long best = ~0ull;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
    if (status[i] != Q_OK) { const unsigned long long v = ((unsigned long long)i << 8) | status[i]; best = v < best ? v : best; }
  if (best != ~0ull) atomicMin(first_bad, best);
}

}  // namespace awry
