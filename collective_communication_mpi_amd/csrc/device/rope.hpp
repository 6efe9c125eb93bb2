// Constants of the rotary position embedding kernels (rope.hip).
#pragma once

#include <stdint.h>

namespace ccmpi {
namespace dev {

constexpr int kRopeThreads = 256;
// Heads whose loads a thread issues before its first store (2 x 16 bytes each).
constexpr int kRopeInFlight = 4;
constexpr int kRopeMaxSeqs = 65536;  // sequences of one packed call

// Head lanes of a token: its threads are (head lane, slice of 8 pairs), lane l walking heads l,
// l + lanes, ... of the concatenated axis [q's heads | k's heads].  Batched: one lane per head up
// to 64; at the Llama-3-8B shape (40 heads, D = 128) that measured 9 % faster than 8 lanes of 5
// heads on a working set beyond the Infinity Cache and 1 % slower inside it.  Packed: a token's
// threads come close to one wave (64 / slices lanes), so that one bisection of cu_seqlens serves
// several heads per thread; with one head per thread the packed mode measured 25 % slower at 64
// documents (profiles/rope/README.md).  Never more lanes than heads.  The results do not depend on
// the choice (every element is computed by itself).
constexpr int kRopeMaxLanes = 64;

inline int64_t rope_head_lanes(int64_t slices, int64_t H, bool packed) {
  int64_t lanes = packed ? kRopeMaxLanes / slices : kRopeMaxLanes;
  if (lanes < 1) lanes = 1;
  return lanes < H ? lanes : H;
}

}  // namespace dev
}  // namespace ccmpi
