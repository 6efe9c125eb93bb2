// Constants of the fused top-k router kernels (moe_gate.hip).
#pragma once

namespace ccmpi {
namespace dev {

constexpr int kGateMaxExperts = 256;  // = kMoeMaxExperts: four experts per lane of a wave
constexpr int kGateMaxTopK = 8;       // = kMoeMaxTopK
// Consecutive tokens per CTA of the forward kernel.  The per-expert probability sums are
// accumulated per chunk and the chunks reduced in order, so this constant (not the grid or
// the scheduling) fixes the summation order of prob_sum: changing it changes its last bits.
constexpr int kGateChunk = 64;

}  // namespace dev
}  // namespace ccmpi
