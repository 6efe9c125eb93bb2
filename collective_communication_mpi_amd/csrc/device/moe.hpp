// Host-visible interface of the routed MoE token dispatch / weighted combine
// kernels and the combine's backward (moe.hip).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "collectives.hpp"

namespace ccmpi {
namespace dev {

constexpr int kMoeMaxExperts = 256;  // one thread of a CTA per expert
constexpr int kMoeMaxTopK = 8;
constexpr int kMoeChunk = 1024;      // (token, slot) entries per routing chunk

// Entries are the flat (token, slot) pairs f = t * K + k of this rank.
struct MoEArgs {
  CollArgs a;              // dispatch: src_code = scratch (count rows), res_code = recv_x, in = x
                           // combine:  src_code = y, out = out
                           // combine backward: src_code = y (0: no dweights), res_code = dy, in = dout
  const int32_t* idx;      // [T * K] expert of each entry, -1 = dropped
  int32_t* row_of;         // [T * K] routing: stable rank among this rank's entries of the same expert;
                           //         dispatch: the row taken in the destination's buffer (in place); -1 = none
  const float* weights;    // combine: [T * K] or null (all ones)
  float* dweights;         // combine backward out: [T * K] <dout[t], y row>, or null (no pull)
  int64_t* expert_counts;  // dispatch out: [E / p] rows per local expert
  int32_t* chunk_hist;     // routing workspace: [chunks][E]
  int32_t* count_row;      // routing out: this rank's staged row at the start of its scratch segment (E int32)
  int32_t T, K, E, El;
  uint32_t row_bytes;      // D * element size, a 16-B multiple
  int32_t cap;             // rows of this rank's recv_x
  int32_t dtype;           // combine: DT_F32 / DT_BF16 / DT_F16
  int32_t expert_cap;      // dispatch: rows kept per expert (the same on every rank), 0 = no limit
  int64_t* num_dropped;    // dispatch out: [1] this rank's entries over expert_cap, or null
};

inline int moe_chunks(int64_t entries) { return (int)((entries + kMoeChunk - 1) / kMoeChunk); }

// routing (local): per-expert counts into count_row, stable per-expert ranks into row_of
void launch_moe_route(const MoEArgs& m, hipStream_t s);
void launch_moe_dispatch(const MoEArgs& m, int grid, hipStream_t s);
void launch_moe_combine(const MoEArgs& m, int grid, hipStream_t s);
void launch_moe_combine_bwd(const MoEArgs& m, int grid, hipStream_t s);

}  // namespace dev
}  // namespace ccmpi
