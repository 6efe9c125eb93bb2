// Fused cross-entropy over a shard of the vocabulary (ops.cross_entropy,
// parallel.vocab_parallel_cross_entropy): logits [T, Vloc] bf16 with unit column stride (row
// stride and Vloc multiples of 8, 16-byte-aligned base), targets [T] int64 in GLOBAL vocabulary
// numbering, vocab_start the global index of column 0.  No fp32 [T, V] tensor exists at any
// point; all address arithmetic is 64-bit; no atomics anywhere.
//
//   k_xent_stats     one read pass.  Workgroup (t, split) covers xent_split_sweeps(T, Vloc)
//                    sweeps of kXentSweep columns of row t: every thread keeps a running
//                    (max, sum of exp(z - max)) over its 16-byte loads, the workgroup takes the
//                    max (fixed xor butterflies, then LDS in wave order), rescales and adds the
//                    sums the same way, and thread 0 writes the partial (m, s, zt, hit) as one
//                    16-byte store into stats[split, t, 0:4]: zt the target's logit (one load,
//                    guarded by the range test, so no content of `targets` makes an address
//                    leave the tensor) and hit = 1 when the target lies in this split's
//                    columns, else both 0.  -inf logits are legal: a partial whose columns are
//                    all -inf is (m = -inf, s = 0), exp(-inf - -inf) is never evaluated.
//   k_xent_combine   thread t merges the row's P partials (TP ranks x splits, rank-major) in
//                    index order: M = max m_i, S = sum s_i exp(m_i - M), lse = M + log S,
//                    zt = sum zt_i; row_loss = lse - zt, exactly 0 where target ==
//                    ignore_index.  The workgroup adds its kXentChunk rows (butterflies, wave
//                    order) into work[chunk] = (loss, valid rows).
//   k_xent_sum       one workgroup adds the chunks: thread j takes chunks j, j + 256, ... in
//                    order, then the same fixed tree: loss_sum [1] fp32, n_valid [1] int64 and
//                    mean [1] = loss_sum / n_valid (0 when n_valid == 0).  The order is fixed by
//                    T alone.
//   k_xent_backward  one read pass, one write pass: dlogits[t, j] = (exp(z - lse[t]) -
//                    [vocab_start + j == target[t]]) * (g / n_valid), the product in fp32,
//                    rounded once to bf16 (nearest even), stored 16 bytes at a time.  g [1]
//                    fp32 and n_valid [1] int64 are read from device memory.  Ignored rows, and
//                    every row when n_valid <= 0, store exact zeros without reading (torch
//                    gives NaN for a mean over no rows; here that mean is 0).  dlogits may BE
//                    logits: every element is read and written by the same thread.
#include <pybind11/pybind11.h>

#include <climits>
#include <cmath>

#include "common.hpp"
#include "ops.hpp"
#include "xent.hpp"

namespace ccmpi {
namespace dev {

namespace {

constexpr int kThreads = kXentThreads;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxPartials = kMaxRanks * kXentMaxSplits;
static_assert(kXentChunk == kThreads, "one row per thread in the combine kernel");

// Fixed butterflies: every lane ends with the same bits, whatever the scheduling.
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor(v, s, 64);
  return v;
}

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor(v, s, 64);
  return v;
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) v = fmaxf(v, __shfl_xor(v, s, 64));
  return v;
}

// exp(d) for d <= 0 (and a few units above): one multiply and v_exp_f32; exp(-inf) = 0.
__device__ __forceinline__ float exp_fast(float d) { return __builtin_amdgcn_exp2f(d * 1.44269504088896341f); }

__device__ __forceinline__ void unpack8(u32x4 v, float (&x)[8]) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    x[2 * i] = bf16_lo(v[i]);
    x[2 * i + 1] = bf16_hi(v[i]);
  }
}

// The workgroup's max / sum of one value per thread, in wave order; every thread gets it.
__device__ __forceinline__ float block_max(float v, float* s_red) {
  v = wave_max(v);
  if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
  __syncthreads();
  float r = s_red[0];
#pragma unroll
  for (int w = 1; w < kWaves; ++w) r = fmaxf(r, s_red[w]);
  __syncthreads();
  return r;
}

__device__ __forceinline__ float block_sum(float v, float* s_red) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
  __syncthreads();
  float r = s_red[0];
#pragma unroll
  for (int w = 1; w < kWaves; ++w) r += s_red[w];
  __syncthreads();
  return r;
}

__global__ void __launch_bounds__(kThreads) k_xent_stats(const uint16_t* __restrict__ logits,
                                                         const int64_t* __restrict__ targets,
                                                         float4* __restrict__ stats, int64_t T, int64_t Vloc,
                                                         int64_t stride, int64_t vocab_start, int64_t per) {
  __shared__ float s_red[kWaves];
  const int64_t t = blockIdx.x, split = blockIdx.y;
  const uint16_t* row = logits + t * stride;
  const int64_t c0 = split * per * kXentSweep;
  const int64_t c1 = min(Vloc, c0 + per * kXentSweep);
  float m = -INFINITY, s = 0.0f;
#pragma unroll 2
  for (int64_t c = c0 + (int64_t)threadIdx.x * 8; c < c1; c += kXentSweep) {
    float x[8];
    unpack8(*reinterpret_cast<const u32x4*>(row + c), x);
    const float vm = fmaxf(fmaxf(fmaxf(x[0], x[1]), fmaxf(x[2], x[3])), fmaxf(fmaxf(x[4], x[5]), fmaxf(x[6], x[7])));
    const float mn = fmaxf(m, vm);
    const float base = mn == -INFINITY ? 0.0f : mn;  // all -inf so far: every term below is exp(-inf) = 0
    float e[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) e[j] = exp_fast(x[j] - base);
    s = s * exp_fast(m - base) + (((e[0] + e[1]) + (e[2] + e[3])) + ((e[4] + e[5]) + (e[6] + e[7])));
    m = mn;
  }
  const float M = block_max(m, s_red);
  const float S = block_sum(s * exp_fast(m - (M == -INFINITY ? 0.0f : M)), s_red);
  if (threadIdx.x == 0) {
    const int64_t tg = targets[t];
    const int64_t col = tg >= vocab_start ? tg - vocab_start : -1;  // vocab_start >= 0: no overflow
    const bool hit = col >= c0 && col < c1;
    float zt = 0.0f;
    if (hit) zt = __uint_as_float((uint32_t)row[col] << 16);
    stats[split * T + t] = make_float4(M, S, zt, hit ? 1.0f : 0.0f);
  }
}

__global__ void __launch_bounds__(kThreads) k_xent_combine(const float4* __restrict__ stats,
                                                           const int64_t* __restrict__ targets,
                                                           float* __restrict__ lse, float* __restrict__ row_loss,
                                                           float* __restrict__ work, int P, int64_t T,
                                                           int64_t ignore_index) {
  __shared__ float s_red[kWaves];
  const int64_t t = (int64_t)blockIdx.x * kXentChunk + threadIdx.x;
  float loss = 0.0f;
  int valid = 0;
  if (t < T) {
    float M = -INFINITY;
    for (int i = 0; i < P; ++i) M = fmaxf(M, stats[(int64_t)i * T + t].x);
    float S = 0.0f, zt = 0.0f;
    for (int i = 0; i < P; ++i) {  // index order
      const float4 q = stats[(int64_t)i * T + t];
      if (q.x != -INFINITY) S += q.y * expf(q.x - M);  // an all -inf partial adds nothing (no inf - inf)
      zt += q.z;
    }
    const float l = M + logf(S);
    valid = targets[t] != ignore_index;
    loss = valid ? l - zt : 0.0f;
    lse[t] = l;
    row_loss[t] = loss;
  }
  const float bl = block_sum(loss, s_red);
  const float bc = block_sum((float)valid, s_red);  // <= 256: exact
  if (threadIdx.x == 0) {
    work[2 * (int64_t)blockIdx.x] = bl;
    work[2 * (int64_t)blockIdx.x + 1] = bc;
  }
}

__global__ void __launch_bounds__(kThreads) k_xent_sum(const float* __restrict__ work, int64_t chunks,
                                                       float* __restrict__ loss_sum, int64_t* __restrict__ n_valid,
                                                       float* __restrict__ mean) {
  __shared__ float s_red[kWaves];
  __shared__ int s_cnt[kWaves];
  float acc = 0.0f;
  int cnt = 0;  // <= T / 256 per thread, < 2^31 per workgroup
  for (int64_t c = threadIdx.x; c < chunks; c += kThreads) {  // chunk order
    acc += work[2 * c];
    cnt += (int)work[2 * c + 1];
  }
  const float total = block_sum(acc, s_red);
  cnt = wave_sum(cnt);
  if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) {
    int64_t n = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) n += s_cnt[w];
    loss_sum[0] = total;
    n_valid[0] = n;
    if (mean != nullptr) mean[0] = n > 0 ? __fdiv_rn(total, (float)n) : 0.0f;
  }
}

// no __restrict__ on logits / dlogits: they may be the same tensor
__global__ void __launch_bounds__(kThreads) k_xent_backward(const uint16_t* logits,
                                                            const int64_t* __restrict__ targets,
                                                            const float* __restrict__ lse,
                                                            const int64_t* __restrict__ n_valid,
                                                            const float* __restrict__ grad, uint16_t* dlogits,
                                                            int64_t Vloc, int64_t in_stride, int64_t out_stride,
                                                            int64_t vocab_start, int64_t ignore_index, int64_t per) {
  const int64_t t = blockIdx.x, split = blockIdx.y;
  const int64_t c0 = split * per * kXentSweep;
  const int64_t c1 = min(Vloc, c0 + per * kXentSweep);
  const uint16_t* row = logits + t * in_stride;
  uint16_t* out = dlogits + t * out_stride;
  const int64_t tg = targets[t];
  const int64_t n = n_valid[0];
  if (tg == ignore_index || n <= 0) {
    for (int64_t c = c0 + (int64_t)threadIdx.x * 8; c < c1; c += kXentSweep)
      *reinterpret_cast<u32x4*>(out + c) = u32x4{0u, 0u, 0u, 0u};
    return;
  }
  const float scale = __fdiv_rn(grad[0], (float)n);
  const float L = lse[t];
  // the target's column of this shard, -1 when it lies elsewhere (vocab_start >= 0: no overflow)
  const int64_t col = tg >= vocab_start && tg - vocab_start < Vloc ? tg - vocab_start : -1;
#pragma unroll 2
  for (int64_t c = c0 + (int64_t)threadIdx.x * 8; c < c1; c += kXentSweep) {
    float x[8];
    unpack8(*reinterpret_cast<const u32x4*>(row + c), x);
#pragma unroll
    for (int j = 0; j < 8; ++j) x[j] = (exp_fast(x[j] - L) - (c + j == col ? 1.0f : 0.0f)) * scale;
    u32x4 v;
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = pk_bf16(x[2 * i], x[2 * i + 1]);
    *reinterpret_cast<u32x4*>(out + c) = v;
  }
}

void check_logits(const char* what, uint64_t ptr, int64_t T, int64_t Vloc, int64_t stride) {
  if (T < 1 || T > INT_MAX) throw std::invalid_argument("xent: 1 <= T < 2^31 required");
  if (Vloc < 8 || Vloc % 8 || Vloc > INT_MAX - kXentSweep)
    throw std::invalid_argument("xent: Vloc must be a positive multiple of 8 below 2^31 - 2048");
  if (stride % 8 || (T > 1 && stride < Vloc))
    throw std::invalid_argument(std::string("xent: the row stride of ") + what + " must be a multiple of 8, >= Vloc");
  if (ptr == 0 || ptr % 16) throw std::invalid_argument(std::string("xent: ") + what + " must be 16-byte aligned");
}

void xent_stats(uint64_t logits, uint64_t targets, uint64_t stats, int64_t T, int64_t Vloc, int64_t stride,
                int64_t vocab_start, int64_t splits, uint64_t stream) {
  check_logits("logits", logits, T, Vloc, stride);
  if (vocab_start < 0 || vocab_start > (int64_t)1 << 62) throw std::invalid_argument("xent: vocab_start out of range");
  if (splits != xent_row_splits(T, Vloc)) throw std::invalid_argument("xent: splits must be xent_row_splits(T, Vloc)");
  if (targets == 0 || targets % 8 || stats == 0 || stats % 16) throw std::invalid_argument("xent: misaligned buffers");
  hipLaunchKernelGGL(k_xent_stats, dim3((unsigned)T, (unsigned)splits), dim3(kThreads), 0,
                     reinterpret_cast<hipStream_t>(stream), reinterpret_cast<const uint16_t*>(logits),
                     reinterpret_cast<const int64_t*>(targets), reinterpret_cast<float4*>(stats), T, Vloc, stride,
                     vocab_start, xent_split_sweeps(T, Vloc));
  CCMPI_HIP_CHECK(hipGetLastError());
}

void xent_combine(uint64_t stats, uint64_t targets, uint64_t lse, uint64_t row_loss, uint64_t loss_sum,
                  uint64_t n_valid, uint64_t mean, uint64_t work, int64_t P, int64_t T, int64_t ignore_index,
                  uint64_t stream) {
  if (T < 1 || T > INT_MAX) throw std::invalid_argument("xent: 1 <= T < 2^31 required");
  if (P < 1 || P > kMaxPartials) throw std::invalid_argument("xent: 1 <= partials <= 1024 required");
  if (stats == 0 || stats % 16 || targets == 0 || targets % 8 || n_valid == 0 || n_valid % 8 || lse == 0 ||
      row_loss == 0 || loss_sum == 0 || work == 0 || (lse | row_loss | loss_sum | mean | work) % 4)
    throw std::invalid_argument("xent: misaligned buffers");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int64_t chunks = (T + kXentChunk - 1) / kXentChunk;
  hipLaunchKernelGGL(k_xent_combine, dim3((unsigned)chunks), dim3(kThreads), 0, st,
                     reinterpret_cast<const float4*>(stats), reinterpret_cast<const int64_t*>(targets),
                     reinterpret_cast<float*>(lse), reinterpret_cast<float*>(row_loss), reinterpret_cast<float*>(work),
                     (int)P, T, ignore_index);
  hipLaunchKernelGGL(k_xent_sum, dim3(1), dim3(kThreads), 0, st, reinterpret_cast<const float*>(work), chunks,
                     reinterpret_cast<float*>(loss_sum), reinterpret_cast<int64_t*>(n_valid),
                     reinterpret_cast<float*>(mean));
  CCMPI_HIP_CHECK(hipGetLastError());
}

void xent_backward(uint64_t logits, uint64_t targets, uint64_t lse, uint64_t n_valid, uint64_t grad, uint64_t dlogits,
                   int64_t T, int64_t Vloc, int64_t in_stride, int64_t out_stride, int64_t vocab_start,
                   int64_t ignore_index, uint64_t stream) {
  check_logits("logits", logits, T, Vloc, in_stride);
  check_logits("dlogits", dlogits, T, Vloc, out_stride);
  if (vocab_start < 0 || vocab_start > (int64_t)1 << 62) throw std::invalid_argument("xent: vocab_start out of range");
  if (targets == 0 || targets % 8 || n_valid == 0 || n_valid % 8 || lse == 0 || lse % 4 || grad == 0 || grad % 4)
    throw std::invalid_argument("xent: misaligned buffers");
  hipLaunchKernelGGL(k_xent_backward, dim3((unsigned)T, (unsigned)xent_row_splits(T, Vloc)), dim3(kThreads), 0,
                     reinterpret_cast<hipStream_t>(stream), reinterpret_cast<const uint16_t*>(logits),
                     reinterpret_cast<const int64_t*>(targets), reinterpret_cast<const float*>(lse),
                     reinterpret_cast<const int64_t*>(n_valid), reinterpret_cast<const float*>(grad),
                     reinterpret_cast<uint16_t*>(dlogits), Vloc, in_stride, out_stride, vocab_start, ignore_index,
                     xent_split_sweeps(T, Vloc));
  CCMPI_HIP_CHECK(hipGetLastError());
}

}  // namespace

void register_xent_ops(pybind11::module_& m) {
  m.attr("XENT_SWEEP") = kXentSweep;
  m.attr("XENT_CHUNK") = kXentChunk;
  m.def("xent_row_splits", [](int64_t T, int64_t Vloc) { return xent_row_splits(T, Vloc); }, pybind11::arg("T"),
        pybind11::arg("Vloc"));
  m.def("xent_stats", &xent_stats,
        "partials (m, s, zt, hit) of logits [T, Vloc] bf16 (row stride in elements) into stats [splits, T, 4] fp32; "
        "targets [T] int64 in global numbering, vocab_start the global index of column 0",
        pybind11::arg("logits"), pybind11::arg("targets"), pybind11::arg("stats"), pybind11::arg("T"),
        pybind11::arg("Vloc"), pybind11::arg("stride"), pybind11::arg("vocab_start"), pybind11::arg("splits"),
        pybind11::arg("stream"), pybind11::call_guard<pybind11::gil_scoped_release>());
  m.def("xent_combine", &xent_combine,
        "merge stats [P, T, 4] in index order: lse [T], row_loss [T], loss_sum [1] fp32, n_valid [1] int64, mean [1] "
        "fp32 (0: none); work: [ceil(T / XENT_CHUNK), 2] fp32 workspace",
        pybind11::arg("stats"), pybind11::arg("targets"), pybind11::arg("lse"), pybind11::arg("row_loss"),
        pybind11::arg("loss_sum"), pybind11::arg("n_valid"), pybind11::arg("mean"), pybind11::arg("work"),
        pybind11::arg("P"), pybind11::arg("T"), pybind11::arg("ignore_index"), pybind11::arg("stream"),
        pybind11::call_guard<pybind11::gil_scoped_release>());
  m.def("xent_backward", &xent_backward,
        "dlogits [T, Vloc] bf16 = (exp(z - lse) - onehot) * grad / n_valid; dlogits may be logits",
        pybind11::arg("logits"), pybind11::arg("targets"), pybind11::arg("lse"), pybind11::arg("n_valid"),
        pybind11::arg("grad"), pybind11::arg("dlogits"), pybind11::arg("T"), pybind11::arg("Vloc"),
        pybind11::arg("in_stride"), pybind11::arg("out_stride"), pybind11::arg("vocab_start"),
        pybind11::arg("ignore_index"), pybind11::arg("stream"), pybind11::call_guard<pybind11::gil_scoped_release>());
}

}  // namespace dev
}  // namespace ccmpi
