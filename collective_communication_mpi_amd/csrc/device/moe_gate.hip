// Fused top-k router of the routed MoE layer (parallel/moe.py RoutedMoE, gate="fused"):
// softmax over the experts, top-k selection, renormalised weights and the two per-expert
// statistics of a load-balancing loss, in one pass over the logits [T, E] (fp32, E <= 256,
// K <= 8); the backward in one more pass.
//
//   k_moe_gate_fwd     one wave per token, lane l holds experts l, l + 64, l + 128, l + 192.
//                      Row max and sum are fixed __shfl_xor butterflies.  Selection runs on the
//                      LOGITS: K rounds of a wave-wide argmax over the key (logit, lower index
//                      wins), the winner removed each round, so idx is exactly the first K
//                      entries of a stable sort by (-logit, index) whatever exp rounds to;
//                      slot order is selection order.  weights[t, k] = p[idx], divided by the
//                      sum of the K selected probabilities (slot order) when renormalising.
//                      -inf logits are legal (probability 0) while a row has a finite one.
//                      CTA c owns the kGateChunk consecutive tokens from c * kGateChunk: wave w
//                      (of 16) takes tokens w, w + 16, ... of the chunk and adds p (and the
//                      selection counts) per lane in token order, the CTA folds its waves in
//                      wave order and writes one [E] row of the partials.
//   k_moe_gate_reduce  thread e adds the partial rows in chunk order: prob_sum[e] (fp32) and
//                      expert_tokens[e] (int64).  No atomics anywhere, so prob_sum is bitwise
//                      reproducible and depends on kGateChunk only.
//   k_moe_gate_bwd     one wave per token; p is recomputed from the logits (nothing of size
//                      [T, E] is saved).  With g = dL/dp: g[e] = dprob_sum[e], plus for the
//                      selected slots dp_k = (dw_k - sum_j dw_j w_j) / S (S = the sum of the
//                      selected p; just dw_k without renormalisation); then
//                      dlogits[t, e] = p_e (g_e - sum_j p_j g_j).  An expert is selected at
//                      most once per token, so the scatter into g has no conflicts.
#include <pybind11/pybind11.h>

#include <climits>
#include <cmath>

#include "common.hpp"
#include "moe_gate.hpp"
#include "ops.hpp"

namespace ccmpi {
namespace dev {

namespace {

constexpr int kThreads = 256;            // backward and reduction
constexpr int kWaves = kThreads / 64;
constexpr int kFwdWaves = 16;            // forward: 16 waves share a chunk, so a wave's serial chain is 4 tokens
constexpr int kFwdThreads = kFwdWaves * 64;
constexpr int kPerLane = kGateMaxExperts / 64;
static_assert(kThreads == kGateMaxExperts, "one thread per expert in the reduction");
static_assert(kFwdThreads >= kGateMaxExperts, "one thread per expert when the waves are folded");
static_assert(kGateChunk % kFwdWaves == 0, "every wave takes the same share of a chunk");

// Fixed butterflies: every lane ends with the same bits, whatever the scheduling.
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor(v, s, 64);
  return v;
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) v = fmaxf(v, __shfl_xor(v, s, 64));
  return v;
}

// x[j] = logit of expert lane + 64 j (-inf past E), p[j] = its softmax probability.
__device__ __forceinline__ void gate_probs(const float* __restrict__ row, int E, int lane, float (&x)[kPerLane],
                                           float (&p)[kPerLane]) {
#pragma unroll
  for (int j = 0; j < kPerLane; ++j) {
    const int e = lane + 64 * j;
    x[j] = e < E ? row[e] : -INFINITY;
  }
  const float m = wave_max(fmaxf(fmaxf(x[0], x[1]), fmaxf(x[2], x[3])));
#pragma unroll
  for (int j = 0; j < kPerLane; ++j) p[j] = expf(x[j] - m);  // exp(-inf) = 0
  const float s = wave_sum(((p[0] + p[1]) + p[2]) + p[3]);
#pragma unroll
  for (int j = 0; j < kPerLane; ++j) p[j] = p[j] / s;
}

// The probability of expert e (wave-uniform, in range), fetched from the lane that holds it.
__device__ __forceinline__ float prob_of(const float (&p)[kPerLane], int e) {
  const int slot = e >> 6;
  const float mine = slot == 0 ? p[0] : slot == 1 ? p[1] : slot == 2 ? p[2] : p[3];
  return __shfl(mine, e & 63, 64);
}

__global__ void __launch_bounds__(kFwdThreads) k_moe_gate_fwd(const float* __restrict__ logits,
                                                              float* __restrict__ weights, int32_t* __restrict__ idx,
                                                              float* __restrict__ part_p, int32_t* __restrict__ part_c,
                                                              int T, int E, int K, int renorm) {
  __shared__ float s_p[kFwdWaves][kGateMaxExperts];
  __shared__ int32_t s_c[kFwdWaves][kGateMaxExperts];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t t0 = (int64_t)blockIdx.x * kGateChunk;
  float acc[kPerLane];
  int cnt[kPerLane];
#pragma unroll
  for (int j = 0; j < kPerLane; ++j) {
    acc[j] = 0.0f;
    cnt[j] = 0;
  }
  for (int i = w; i < kGateChunk; i += kFwdWaves) {
    const int64_t t = t0 + i;
    if (t >= T) break;
    float x[kPerLane], p[kPerLane];
    gate_probs(logits + t * E, E, lane, x, p);
#pragma unroll
    for (int j = 0; j < kPerLane; ++j) acc[j] += p[j];
    unsigned removed = 0;
    float wsel[kGateMaxTopK];
    float my_w = 0.0f;
    int my_i = 0;
#pragma unroll
    for (int k = 0; k < kGateMaxTopK; ++k) {
      wsel[k] = 0.0f;
      if (k < K) {
        // the best of this lane's experts, then of the wave: larger logit, then lower index
        float bv = -INFINITY;
        int bi = INT_MAX;
#pragma unroll
        for (int j = 0; j < kPerLane; ++j) {
          const int e = lane + 64 * j;
          const bool cand = e < E && !((removed >> j) & 1u);
          if (cand && (x[j] > bv || (x[j] == bv && e < bi))) {
            bv = x[j];
            bi = e;
          }
        }
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) {
          const float ov = __shfl_xor(bv, s, 64);
          const int oi = __shfl_xor(bi, s, 64);
          if (ov > bv || (ov == bv && oi < bi)) {
            bv = ov;
            bi = oi;
          }
        }
        // K <= E, so a candidate was left: 0 <= win < E (a row with a NaN is unspecified; the
        // clamp only keeps the lane arithmetic below in range then)
        const int win = min(max(__builtin_amdgcn_readfirstlane(bi), 0), E - 1);
        wsel[k] = prob_of(p, win);
        if (lane == (win & 63)) {
          removed |= 1u << (win >> 6);
#pragma unroll
          for (int j = 0; j < kPerLane; ++j) cnt[j] += (win >> 6) == j;
        }
        if (lane == k) {
          my_w = wsel[k];
          my_i = win;
        }
      }
    }
    float S = 0.0f;
#pragma unroll
    for (int k = 0; k < kGateMaxTopK; ++k)
      if (k < K) S += wsel[k];  // slot order
    if (lane < K) {
      weights[t * K + lane] = renorm ? my_w / S : my_w;
      idx[t * K + lane] = my_i;
    }
  }
#pragma unroll
  for (int j = 0; j < kPerLane; ++j) {
    s_p[w][lane + 64 * j] = acc[j];
    s_c[w][lane + 64 * j] = cnt[j];
  }
  __syncthreads();
  const int e = threadIdx.x;
  if (e < E) {
    float sp = s_p[0][e];
    int sc = s_c[0][e];
#pragma unroll
    for (int ww = 1; ww < kFwdWaves; ++ww) {  // wave order
      sp += s_p[ww][e];
      sc += s_c[ww][e];
    }
    part_p[(int64_t)blockIdx.x * E + e] = sp;
    part_c[(int64_t)blockIdx.x * E + e] = sc;
  }
}

__global__ void __launch_bounds__(kThreads) k_moe_gate_reduce(const float* __restrict__ part_p,
                                                              const int32_t* __restrict__ part_c,
                                                              float* __restrict__ prob_sum,
                                                              int64_t* __restrict__ expert_tokens, int chunks, int E) {
  const int e = threadIdx.x;
  if (e >= E) return;
  float sp = 0.0f;
  int64_t sc = 0;
  constexpr int B = 16;  // loads in flight; the adds stay in chunk order
  for (int c0 = 0; c0 < chunks; c0 += B) {
    float a[B];
    int32_t b[B];
#pragma unroll
    for (int u = 0; u < B; ++u) {
      if (c0 + u < chunks) {
        a[u] = part_p[(int64_t)(c0 + u) * E + e];
        b[u] = part_c[(int64_t)(c0 + u) * E + e];
      }
    }
#pragma unroll
    for (int u = 0; u < B; ++u) {
      if (c0 + u < chunks) {
        sp += a[u];
        sc += b[u];
      }
    }
  }
  prob_sum[e] = sp;
  expert_tokens[e] = sc;
}

__global__ void __launch_bounds__(kThreads) k_moe_gate_bwd(const float* __restrict__ logits,
                                                           const int32_t* __restrict__ idx,
                                                           const float* __restrict__ dweights,
                                                           const float* __restrict__ dprob_sum,
                                                           float* __restrict__ dlogits, int T, int E, int K,
                                                           int renorm) {
  const int lane = threadIdx.x & 63;
  const int64_t t = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (t >= T) return;
  float x[kPerLane], p[kPerLane], g[kPerLane];
  gate_probs(logits + t * E, E, lane, x, p);
#pragma unroll
  for (int j = 0; j < kPerLane; ++j) {
    const int e = lane + 64 * j;
    g[j] = dprob_sum != nullptr && e < E ? dprob_sum[e] : 0.0f;
  }
  int sel[kGateMaxTopK];
  float dw[kGateMaxTopK], ps[kGateMaxTopK];
  float S = 0.0f;
#pragma unroll
  for (int k = 0; k < kGateMaxTopK; ++k) {
    sel[k] = -1;
    dw[k] = ps[k] = 0.0f;
    if (k < K) {
      const int e = __builtin_amdgcn_readfirstlane(idx[t * K + k]);
      if (e >= 0 && e < E) {  // anything else is not a selection of the forward: no gradient
        sel[k] = e;
        dw[k] = dweights[t * K + k];
        ps[k] = prob_of(p, e);
        S += ps[k];  // slot order, as in the forward
      }
    }
  }
  float c = 0.0f;
  if (renorm) {
#pragma unroll
    for (int k = 0; k < kGateMaxTopK; ++k)
      if (k < K) c += dw[k] * (ps[k] / S);
  }
#pragma unroll
  for (int k = 0; k < kGateMaxTopK; ++k) {
    if (k < K && sel[k] >= 0) {
      const float dp = renorm ? (dw[k] - c) / S : dw[k];
      if (lane == (sel[k] & 63)) {
#pragma unroll
        for (int j = 0; j < kPerLane; ++j)
          if ((sel[k] >> 6) == j) g[j] += dp;
      }
    }
  }
  float dot = 0.0f;
#pragma unroll
  for (int j = 0; j < kPerLane; ++j) dot = __builtin_fmaf(p[j], g[j], dot);
  dot = wave_sum(dot);
#pragma unroll
  for (int j = 0; j < kPerLane; ++j) {
    const int e = lane + 64 * j;
    if (e < E) dlogits[t * E + e] = p[j] * (g[j] - dot);
  }
}

void check_shape(int64_t T, int E, int K) {
  if (E < 1 || E > kGateMaxExperts) throw std::invalid_argument("moe_gate: 1 <= E <= 256 required");
  if (K < 1 || K > kGateMaxTopK || K > E) throw std::invalid_argument("moe_gate: 1 <= top_k <= min(8, E) required");
  if (T < 0 || T > INT_MAX - kGateChunk) throw std::invalid_argument("moe_gate: 0 <= T < 2^31 - 64 required");
}

void moe_gate_fwd(uint64_t logits, uint64_t weights, uint64_t idx, uint64_t part_p, uint64_t part_c,
                  uint64_t prob_sum, uint64_t expert_tokens, int64_t T, int E, int K, bool renorm, uint64_t stream) {
  check_shape(T, E, K);
  if ((logits | weights | idx | part_p | part_c | prob_sum) % 4 || expert_tokens % 8)
    throw std::invalid_argument("moe_gate: misaligned buffers");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int chunks = (int)((T + kGateChunk - 1) / kGateChunk);
  if (chunks)
    hipLaunchKernelGGL(k_moe_gate_fwd, dim3(chunks), dim3(kFwdThreads), 0, st, reinterpret_cast<const float*>(logits),
                       reinterpret_cast<float*>(weights), reinterpret_cast<int32_t*>(idx),
                       reinterpret_cast<float*>(part_p), reinterpret_cast<int32_t*>(part_c), (int)T, E, K,
                       renorm ? 1 : 0);
  hipLaunchKernelGGL(k_moe_gate_reduce, dim3(1), dim3(kThreads), 0, st, reinterpret_cast<const float*>(part_p),
                     reinterpret_cast<const int32_t*>(part_c), reinterpret_cast<float*>(prob_sum),
                     reinterpret_cast<int64_t*>(expert_tokens), chunks, E);
  CCMPI_HIP_CHECK(hipGetLastError());
}

void moe_gate_bwd(uint64_t logits, uint64_t idx, uint64_t dweights, uint64_t dprob_sum, uint64_t dlogits, int64_t T,
                  int E, int K, bool renorm, uint64_t stream) {
  check_shape(T, E, K);
  if ((logits | idx | dweights | dprob_sum | dlogits) % 4) throw std::invalid_argument("moe_gate: misaligned buffers");
  if (T == 0) return;
  hipLaunchKernelGGL(k_moe_gate_bwd, dim3((unsigned)((T + kWaves - 1) / kWaves)), dim3(kThreads), 0,
                     reinterpret_cast<hipStream_t>(stream), reinterpret_cast<const float*>(logits),
                     reinterpret_cast<const int32_t*>(idx), reinterpret_cast<const float*>(dweights),
                     reinterpret_cast<const float*>(dprob_sum), reinterpret_cast<float*>(dlogits), (int)T, E, K,
                     renorm ? 1 : 0);
  CCMPI_HIP_CHECK(hipGetLastError());
}

}  // namespace

void register_moe_gate_ops(pybind11::module_& m) {
  m.attr("MOE_GATE_CHUNK") = kGateChunk;
  m.def("moe_gate_fwd", &moe_gate_fwd,
        "softmax + top-k over logits [T, E] fp32: weights [T, K], idx [T, K] int32, prob_sum [E], expert_tokens [E] "
        "int64; part_p / part_c: [ceil(T / MOE_GATE_CHUNK), E] fp32 / int32 workspaces",
        pybind11::arg("logits"), pybind11::arg("weights"), pybind11::arg("idx"), pybind11::arg("part_p"),
        pybind11::arg("part_c"), pybind11::arg("prob_sum"), pybind11::arg("expert_tokens"), pybind11::arg("T"),
        pybind11::arg("E"), pybind11::arg("K"), pybind11::arg("renorm"), pybind11::arg("stream"),
        pybind11::call_guard<pybind11::gil_scoped_release>());
  m.def("moe_gate_bwd", &moe_gate_bwd,
        "dlogits [T, E] from the logits, the forward's idx, dweights [T, K] and dprob_sum [E] (0: none)",
        pybind11::arg("logits"), pybind11::arg("idx"), pybind11::arg("dweights"), pybind11::arg("dprob_sum"),
        pybind11::arg("dlogits"), pybind11::arg("T"), pybind11::arg("E"), pybind11::arg("K"), pybind11::arg("renorm"),
        pybind11::arg("stream"), pybind11::call_guard<pybind11::gil_scoped_release>());
}

}  // namespace dev
}  // namespace ccmpi
