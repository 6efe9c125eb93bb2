// Constants of the optimizer kernels (optim.hip).
#pragma once

#include <stdint.h>

namespace ccmpi {
namespace dev {

constexpr int kOptimThreads = 256;
// Elements of one slot: 256 threads x 8 (ops.OPTIM_CHUNK mirrors this).  A pure constant, never a
// function of the device: the slot map fixes the order of the norm's additions.
constexpr int kOptimChunk = kOptimThreads * 8;
// Workgroups of one launch, at most; a workgroup walks the slots wg, wg + grid, ...
constexpr int kOptimMaxGrid = 4096;
// Threads of k_optim_sums' one workgroup: thread t adds the partials t, t + 1024, ...
constexpr int kOptimSumThreads = 1024;
constexpr int64_t kOptimMaxSegs = (int64_t)1 << 24;
constexpr int64_t kOptimMaxElems = (int64_t)1 << 40;

// segment flags
constexpr int kOptimDecay = 1;    // weight decay applies
constexpr int kOptimSharded = 2;  // counted in the "sharded" norm sum

inline int64_t optim_slots(int64_t n, int64_t S) { return n / kOptimChunk + S; }

}  // namespace dev
}  // namespace ccmpi
