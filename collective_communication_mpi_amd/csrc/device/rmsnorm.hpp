// Constants of the RMSNorm kernels (rmsnorm.hip).
#pragma once

#include <stdint.h>

namespace ccmpi {
namespace dev {

constexpr int kRmsThreads = 256;
constexpr int kRmsMaxD = 16384;
// 8-element slices of a row that one thread owns, at most: slices t, t + 256, ... of d / 8.
constexpr int kRmsMaxSlices = kRmsMaxD / 8 / kRmsThreads;
constexpr int64_t kRmsMaxRows = (int64_t)1 << 30;

// Rows per workgroup of the backward (ops.rms_norm_row_chunk mirrors this; the launcher uses it).
// A pure function of (T, d), never of the device or the grid: a chunk's rows are added into dw's
// partial in row order and the partials in a fixed order, so the rule is part of dw's bits.  Small
// enough that 4096 tokens give 512 workgroups (two per CU), large enough that the partials
// ([chunks, d] fp32, written once and read once) are at most a sixth of the rows' own traffic.
constexpr int kRmsMinChunk = 8;
constexpr int kRmsMaxChunk = 32;
constexpr int kRmsTargetGroups = 1024;

inline int64_t rms_norm_row_chunk(int64_t T, int64_t /*d*/) {
  int64_t c = (T + kRmsTargetGroups - 1) / kRmsTargetGroups;
  if (c < kRmsMinChunk) c = kRmsMinChunk;
  if (c > kRmsMaxChunk) c = kRmsMaxChunk;
  return c;
}

// k_rmsnorm_dw: a workgroup owns kRmsDwCols columns; chunk lane l of kRmsDwLanes adds the chunks
// l, l + kRmsDwLanes, ... in that order, then the lanes are added in lane order.
constexpr int kRmsDwCols = 32;
constexpr int kRmsDwLanes = 32;

}  // namespace dev
}  // namespace ccmpi
