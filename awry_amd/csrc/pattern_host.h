// pattern_host.h -- host batch drivers of class-pattern count and locate (pattern_kernels.hip.h)
// A part of awry_hip.hip (one translation unit): included there, in order, and not on its own.
#pragma once

namespace {

static_assert(PT_MAX_CLASS == AWRY_MAX_CLASS_POSITIONS && PT_MAX_FRAMES == AWRY_PATTERN_MAX_FRAMES && MM_MAX_K == AWRY_MAX_MISMATCHES,
              "the kernel's limits are the header's");
static_assert(Q_NOT_CLASS_LETTER == AWRY_Q_NOT_CLASS_LETTER && Q_CLASS_POSITIONS == AWRY_Q_CLASS_POSITIONS && Q_EXPANSION_CAP == AWRY_Q_EXPANSION_CAP,
              "the kernel's status bytes are the header's");

// Everything after the leaves is the mismatch path's (mismatch_host.h): chunking, the shared leaf cap, segmented sort by first
// row, launch_locate, per-hit distance.  Patterns are validated where they are searched (lane refill of the kernel), and a
// rejected or abandoned pattern fails the batch through its status byte, before any result array is handed out.
void count_pattern_batch(awry_index* idx, const uint8_t* qbytes, const uint64_t* qoff, uint64_t n, int k, uint64_t* counts_out) {
  count_leaves_batch(idx, qbytes, qoff, n, k, counts_out, launch_count_pattern);
}

void locate_pattern_batch(awry_index* idx, const uint8_t* qbytes, const uint64_t* qoff, uint64_t n, int k, uint64_t** hit_off_out,
                          awry_pos_t** hits_out, uint64_t** global_pos_out, uint8_t** mismatches_out) {
  locate_leaves_batch(idx, qbytes, qoff, n, k, hit_off_out, hits_out, global_pos_out, mismatches_out, launch_count_pattern);
}

}  // namespace
