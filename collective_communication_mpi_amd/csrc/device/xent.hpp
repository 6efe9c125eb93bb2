// Constants of the fused cross-entropy kernels (xent.hip).
#pragma once

#include <stdint.h>

namespace ccmpi {
namespace dev {

constexpr int kXentThreads = 256;
// Columns one workgroup covers per sweep: 256 threads x one 16-byte load of 8 bf16.
constexpr int kXentSweep = kXentThreads * 8;
// Rows per workgroup of the combine kernel.  loss_sum adds the rows of a chunk in a fixed tree
// and the chunks in a fixed order, so this constant and T alone fix its summation order.
constexpr int kXentChunk = 256;
// Column splits of one row (ops.xent_row_splits mirrors this): small T with a large shard
// still fills the chip.  A pure function of (T, Vloc) -- never of the device or the grid --
// because every split writes a partial of its own and the merge order is part of the bits.
constexpr int kXentTargetGroups = 1024;  // workgroups wanted in flight
constexpr int kXentMinSweeps = 4;        // a split keeps at least this many sweeps
constexpr int kXentMaxSplits = 64;

inline int64_t xent_sweeps(int64_t Vloc) { return (Vloc + kXentSweep - 1) / kXentSweep; }

// sweeps per split, then the number of (non-empty) splits
inline int64_t xent_split_sweeps(int64_t T, int64_t Vloc) {
  const int64_t n = xent_sweeps(Vloc);
  int64_t want = T >= kXentTargetGroups ? 1 : (kXentTargetGroups + T - 1) / T;
  if (want > n / kXentMinSweeps) want = n / kXentMinSweeps;
  if (want > kXentMaxSplits) want = kXentMaxSplits;
  if (want < 1) want = 1;
  return (n + want - 1) / want;
}

inline int64_t xent_row_splits(int64_t T, int64_t Vloc) {
  const int64_t per = xent_split_sweeps(T, Vloc);
  return (xent_sweeps(Vloc) + per - 1) / per;
}

}  // namespace dev
}  // namespace ccmpi
