// RMSNorm with the residual add in front of it (ops.rms_norm, ops.add_rms_norm): x and, optionally,
// residual [T, d] bf16; h = bf16(x + residual) (one fp32 add, rounded once: torch's bf16 add), or
// h = x; rstd[t] = 1 / sqrt(mean_j h[t, j]^2 + eps) fp32; y[t, j] = bf16(h[t, j] rstd[t] w[j]).
// Backward, with n = h rstd and g = dy w: dh = bf16(rstd (g - n mean_k(g n)) + dres), dw[j] =
// sum_t dy[t, j] n[t, j] in fp32.  bf16 in and out, fp32 arithmetic, one rounding per output
// element, no atomics, all address arithmetic 64-bit.  Every [T, d] operand is a view with a row
// stride of its own (unit column stride, row stride a multiple of 8 elements, 16-byte-aligned
// base); w is [d] bf16 or fp32, contiguous.  8 <= d <= 16384, d % 8 == 0, 1 <= T <= 2^30.
//
// Mapping, all kernels: a row's d / 8 slices of 8 elements (16 bytes) are dealt to the 256 threads
// of ONE workgroup, thread t owning slices t, t + 256, ... (NS of them at most, a template
// argument chosen from d alone), so a wave-wide access covers 1 KiB of one row.  A thread reads
// all it owns of a row, of every operand, before it writes any of it: an output may BE an input
// (h over x or residual, dh over dy or dres), as the same view.
//
//   k_rmsnorm_fwd  workgroup = row.  The row is read once and kept in registers (packed bf16)
//                  between the sum of squares and the scaling; h is stored once more with a
//                  residual.  The sum's order depends on d alone: a thread's FMA chain over its
//                  slices in slice order (64 deep at most), the xor butterfly of its wave, then
//                  (w0 + w1) + (w2 + w3) through LDS: 72 dependent additions at most.  A row's y,
//                  h and rstd therefore do not depend on T or on the other rows.
//   k_rmsnorm_bwd  workgroup = rms_norm_row_chunk(T, d) consecutive rows, walked in order, w in
//                  registers.  Per row: n from h and rstd, one workgroup sum for mean(g n) (one
//                  barrier: the LDS slots alternate), dh stored.  DW: per-thread fp32
//                  accumulators add dy n for the thread's columns in row order and end in
//                  partials[chunk, 0:d].
//   k_rmsnorm_dw   partials [chunks, d] -> dw [d]: chunk lane l of 32 adds the chunks l, l + 32,
//                  ... in that order, then the lanes are added in lane order.  The order is
//                  fixed by (T, d): dw is bitwise reproducible on any device.
#include <hip/hip_runtime.h>
#include <pybind11/pybind11.h>

#include <cmath>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <utility>

#include "common.hpp"
#include "ops.hpp"
#include "rmsnorm.hpp"

namespace ccmpi {
namespace dev {

namespace {

constexpr int kThreads = kRmsThreads;
constexpr int kWaves = kThreads / 64;
static_assert(kWaves == 4, "the wave tree below is (w0 + w1) + (w2 + w3)");
static_assert(kRmsDwCols * kRmsDwLanes == 4 * kThreads, "k_rmsnorm_dw: one float4 per thread and step");

// The arithmetic, spelled with intrinsics so that no instantiation contracts differently.
__device__ __forceinline__ float add_residual(float x, float r) { return __fadd_rn(x, r); }
__device__ __forceinline__ float square_acc(float v, float acc) { return __fmaf_rn(v, v, acc); }
__device__ __forceinline__ float rstd_of(float ss, float d, float eps) {
  return __fdiv_rn(1.0f, __fsqrt_rn(__fadd_rn(__fdiv_rn(ss, d), eps)));
}
__device__ __forceinline__ float normalise(float h, float rstd) { return __fmul_rn(h, rstd); }
__device__ __forceinline__ float scale(float n, float w) { return __fmul_rn(n, w); }
// dh before its rounding: rstd (g - n c) + dres, c = mean(g n)
__device__ __forceinline__ float input_grad(float g, float n, float c, float rstd, float dres) {
  return __fmaf_rn(rstd, __fmaf_rn(-n, c, g), dres);
}

__device__ __forceinline__ void unpack8(u32x4 v, float (&x)[8]) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    x[2 * i] = bf16_lo(v[i]);
    x[2 * i + 1] = bf16_hi(v[i]);
  }
}

__device__ __forceinline__ u32x4 pack8(const float (&x)[8]) {
  u32x4 v;
#pragma unroll
  for (int i = 0; i < 4; ++i) v[i] = pk_bf16(x[2 * i], x[2 * i + 1]);
  return v;
}

// w[col .. col + 8) as fp32: one 16-byte load of bf16, or two of fp32 (f32 is the same in every thread)
__device__ __forceinline__ void load_w8(const void* w, int f32, int col, float (&o)[8]) {
  if (f32) {
    const float* p = static_cast<const float*>(w) + col;
    const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
    o[0] = a.x, o[1] = a.y, o[2] = a.z, o[3] = a.w, o[4] = b.x, o[5] = b.y, o[6] = b.z, o[7] = b.w;
  } else {
    unpack8(*reinterpret_cast<const u32x4*>(static_cast<const uint16_t*>(w) + col), o);
  }
}

// The workgroup's sum of one value per thread: a fixed butterfly, then a fixed tree over the waves.
// ONE barrier: the caller alternates the slot (s_red + 0 / + kWaves) between consecutive sums, and
// a wave that writes a slot again has passed the barrier of the sum in between, which every wave
// reaches only after its reads of that slot.
__device__ __forceinline__ float block_sum(float v, float* s_red) {
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor(v, s, 64);
  if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
  __syncthreads();
  return __fadd_rn(__fadd_rn(s_red[0], s_red[1]), __fadd_rn(s_red[2], s_red[3]));
}

struct RmsFwdArgs {
  const uint16_t* x;
  const uint16_t* res;  // nullptr: h = x, nothing stored to h
  uint16_t* h;
  uint16_t* y;
  const void* w;
  float* rstd;
  int64_t sx, sr, sh, sy;  // row strides in elements
  int d, w_f32;
  float eps;
};

// no __restrict__ on the rows: h may be x or res
template <int NS>
__global__ void __launch_bounds__(kThreads) k_rmsnorm_fwd(const RmsFwdArgs p) {
  __shared__ float s_red[kWaves];
  const int64_t row = blockIdx.x;
  const int slices = p.d >> 3;
  const uint16_t* x = p.x + row * p.sx;
  u32x4 hv[NS];
#pragma unroll
  for (int i = 0; i < NS; ++i) {
    const int s = threadIdx.x + i * kThreads;
    if (s < slices) hv[i] = *reinterpret_cast<const u32x4*>(x + 8 * s);
  }
  if (p.res != nullptr) {
    const uint16_t* r = p.res + row * p.sr;
    uint16_t* h = p.h + row * p.sh;
    u32x4 rv[NS];
#pragma unroll
    for (int i = 0; i < NS; ++i) {
      const int s = threadIdx.x + i * kThreads;
      if (s < slices) rv[i] = *reinterpret_cast<const u32x4*>(r + 8 * s);
    }
#pragma unroll
    for (int i = 0; i < NS; ++i) {
      const int s = threadIdx.x + i * kThreads;
      if (s < slices) {
        float a[8], b[8];
        unpack8(hv[i], a);
        unpack8(rv[i], b);
#pragma unroll
        for (int j = 0; j < 8; ++j) a[j] = add_residual(a[j], b[j]);
        hv[i] = pack8(a);  // everything below sees the ROUNDED h
        *reinterpret_cast<u32x4*>(h + 8 * s) = hv[i];
      }
    }
  }
  float ss = 0.0f;
#pragma unroll
  for (int i = 0; i < NS; ++i) {  // slice order
    const int s = threadIdx.x + i * kThreads;
    if (s < slices) {
      float a[8];
      unpack8(hv[i], a);
#pragma unroll
      for (int j = 0; j < 8; ++j) ss = square_acc(a[j], ss);
    }
  }
  const float rstd = rstd_of(block_sum(ss, s_red), (float)p.d, p.eps);
  if (threadIdx.x == 0) p.rstd[row] = rstd;
  uint16_t* y = p.y + row * p.sy;
#pragma unroll
  for (int i = 0; i < NS; ++i) {
    const int s = threadIdx.x + i * kThreads;
    if (s < slices) {
      float a[8], w[8];
      unpack8(hv[i], a);
      load_w8(p.w, p.w_f32, 8 * s, w);
#pragma unroll
      for (int j = 0; j < 8; ++j) a[j] = scale(normalise(a[j], rstd), w[j]);
      *reinterpret_cast<u32x4*>(y + 8 * s) = pack8(a);
    }
  }
}

struct RmsBwdArgs {
  const uint16_t* dy;
  const uint16_t* h;
  const uint16_t* dres;  // nullptr: zeros
  uint16_t* dh;
  const void* w;
  const float* rstd;
  float* partials;  // DW: [chunks, d]
  int64_t sdy, sh, sdres, sdh;
  int64_t T;
  int d, chunk, w_f32;
};

// no __restrict__ on the rows: dh may be dy or dres
template <int NS, bool DW>
__global__ void __launch_bounds__(kThreads) k_rmsnorm_bwd(const RmsBwdArgs p) {
  __shared__ float s_red[2 * kWaves];
  const int slices = p.d >> 3;
  const int64_t row0 = (int64_t)blockIdx.x * p.chunk;
  const int64_t row1 = row0 + p.chunk < p.T ? row0 + p.chunk : p.T;
  const float fd = (float)p.d;
  float w[NS][8], acc[DW ? NS : 1][8];
#pragma unroll
  for (int i = 0; i < NS; ++i) {
    const int s = threadIdx.x + i * kThreads;
    if (s < slices) load_w8(p.w, p.w_f32, 8 * s, w[i]);
  }
#pragma unroll
  for (int i = 0; i < (DW ? NS : 1); ++i)
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[i][j] = 0.0f;
  for (int64_t row = row0; row < row1; ++row) {  // row order
    const uint16_t* dy = p.dy + row * p.sdy;
    const uint16_t* h = p.h + row * p.sh;
    u32x4 hv[NS], gv[NS], rv[NS];
#pragma unroll
    for (int i = 0; i < NS; ++i) {
      const int s = threadIdx.x + i * kThreads;
      rv[i] = u32x4{0u, 0u, 0u, 0u};  // dres = None is dres = +0: the same bits by construction
      if (s < slices) {
        hv[i] = *reinterpret_cast<const u32x4*>(h + 8 * s);
        gv[i] = *reinterpret_cast<const u32x4*>(dy + 8 * s);
        if (p.dres != nullptr) rv[i] = *reinterpret_cast<const u32x4*>(p.dres + row * p.sdres + 8 * s);
      }
    }
    const float rstd = p.rstd[row];
    float part = 0.0f;
#pragma unroll
    for (int i = 0; i < NS; ++i) {  // slice order
      const int s = threadIdx.x + i * kThreads;
      if (s < slices) {
        float a[8], g[8];
        unpack8(hv[i], a);
        unpack8(gv[i], g);
#pragma unroll
        for (int j = 0; j < 8; ++j) part = __fmaf_rn(scale(g[j], w[i][j]), normalise(a[j], rstd), part);
      }
    }
    const float c = __fdiv_rn(block_sum(part, s_red + ((row - row0) & 1) * kWaves), fd);
    uint16_t* dh = p.dh + row * p.sdh;
#pragma unroll
    for (int i = 0; i < NS; ++i) {
      const int s = threadIdx.x + i * kThreads;
      if (s < slices) {
        float a[8], g[8], r[8];
        unpack8(hv[i], a);
        unpack8(gv[i], g);
        unpack8(rv[i], r);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float n = normalise(a[j], rstd);
          if (DW) acc[i][j] = __fmaf_rn(g[j], n, acc[i][j]);
          a[j] = input_grad(scale(g[j], w[i][j]), n, c, rstd, r[j]);
        }
        *reinterpret_cast<u32x4*>(dh + 8 * s) = pack8(a);
      }
    }
  }
  if (DW) {
    float* out = p.partials + (int64_t)blockIdx.x * p.d;
#pragma unroll
    for (int i = 0; i < (DW ? NS : 1); ++i) {
      const int s = threadIdx.x + i * kThreads;
      if (s < slices) {
        *reinterpret_cast<float4*>(out + 8 * s) = make_float4(acc[i][0], acc[i][1], acc[i][2], acc[i][3]);
        *reinterpret_cast<float4*>(out + 8 * s + 4) = make_float4(acc[i][4], acc[i][5], acc[i][6], acc[i][7]);
      }
    }
  }
}

__global__ void __launch_bounds__(kThreads) k_rmsnorm_dw(const float* __restrict__ partials, float* __restrict__ dw,
                                                         int64_t chunks, int d) {
  __shared__ __attribute__((aligned(16))) float s_part[kRmsDwLanes][kRmsDwCols];
  const int lane = threadIdx.x / (kRmsDwCols / 4), c4 = threadIdx.x % (kRmsDwCols / 4);
  const int col = blockIdx.x * kRmsDwCols + 4 * c4;  // d % 4 == 0: a float4 is inside the row or outside it
  float4 a = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  if (col < d) {
#pragma unroll 4
    for (int64_t c = lane; c < chunks; c += kRmsDwLanes) {  // this lane's chunks, in order
      const float4 v = *reinterpret_cast<const float4*>(partials + c * d + col);
      a.x = __fadd_rn(a.x, v.x), a.y = __fadd_rn(a.y, v.y), a.z = __fadd_rn(a.z, v.z), a.w = __fadd_rn(a.w, v.w);
    }
  }
  *reinterpret_cast<float4*>(&s_part[lane][4 * c4]) = a;
  __syncthreads();
  const int out = blockIdx.x * kRmsDwCols + threadIdx.x;
  if (threadIdx.x < kRmsDwCols && out < d) {
    float r = s_part[0][threadIdx.x];
#pragma unroll
    for (int l = 1; l < kRmsDwLanes; ++l) r = __fadd_rn(r, s_part[l][threadIdx.x]);  // lane order
    dw[out] = r;
  }
}

[[noreturn]] void refuse(const std::string& what) { throw std::invalid_argument("rms_norm: " + what); }

// (address, row stride in elements; 0 for T = 1); (0, 0): absent
using View = std::pair<uint64_t, int64_t>;

void check_shape(int64_t T, int64_t d) {
  if (d < 8 || d > kRmsMaxD || d % 8) refuse("d must be a multiple of 8 in [8, 16384]");
  if (T < 1 || T > kRmsMaxRows) refuse("1 <= T <= 2^30 required");
}

void check_view(const char* what, const View& v) {
  if (v.first == 0 || v.first % 16) refuse(std::string(what) + " must be 16-byte aligned");
  if (v.second % 8) refuse(std::string("the row stride of ") + what + " must be a multiple of 8 elements");
}

void check_buffer(const char* what, uint64_t ptr, int align) {
  if (ptr == 0 || ptr % align) refuse(std::string(what) + " must be " + std::to_string(align) + "-byte aligned");
}

template <typename F>
void for_slices(int64_t d, F&& f) {  // NS from d alone
  const int64_t per = (d / 8 + kThreads - 1) / kThreads;
  if (per <= 1) f(std::integral_constant<int, 1>{});
  else if (per <= 2) f(std::integral_constant<int, 2>{});
  else if (per <= 4) f(std::integral_constant<int, 4>{});
  else f(std::integral_constant<int, kRmsMaxSlices>{});
}

void rms_norm_fwd(View x, View res, View h, View y, uint64_t w, bool w_f32, uint64_t rstd, int64_t T, int64_t d,
                  double eps, uint64_t stream) {
  check_shape(T, d);
  if (!(eps > 0.0) || !std::isfinite(eps) || !((float)eps > 0.0f)) refuse("eps must be a positive float");
  check_view("x", x);
  check_view("y", y);
  if ((res.first == 0) != (h.first == 0)) refuse("residual and h come together");
  if (res.first) {
    check_view("residual", res);
    check_view("h", h);
  }
  check_buffer("weight", w, 16);
  check_buffer("rstd", rstd, 4);
  RmsFwdArgs a{reinterpret_cast<const uint16_t*>(x.first), reinterpret_cast<const uint16_t*>(res.first),
               reinterpret_cast<uint16_t*>(h.first), reinterpret_cast<uint16_t*>(y.first),
               reinterpret_cast<const void*>(w), reinterpret_cast<float*>(rstd), x.second, res.second, h.second,
               y.second, (int)d, w_f32 ? 1 : 0, (float)eps};
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  for_slices(d, [&](auto ns) {
    hipLaunchKernelGGL((k_rmsnorm_fwd<decltype(ns)::value>), dim3((unsigned)T), dim3(kThreads), 0, st, a);
  });
  CCMPI_HIP_CHECK(hipGetLastError());
}

void rms_norm_bwd(View dy, View h, View dres, View dh, uint64_t w, bool w_f32, uint64_t rstd, uint64_t partials,
                  uint64_t dw, int64_t T, int64_t d, int64_t chunk, uint64_t stream) {
  check_shape(T, d);
  if (chunk != rms_norm_row_chunk(T, d)) refuse("chunk must be rms_norm_row_chunk(T, d)");
  check_view("dy", dy);
  check_view("h", h);
  if (dres.first) check_view("dres", dres);
  check_view("dh", dh);
  check_buffer("weight", w, 16);
  check_buffer("rstd", rstd, 4);
  if ((dw == 0) != (partials == 0)) refuse("dw and partials come together");
  if (dw) {
    check_buffer("partials", partials, 16);
    check_buffer("dw", dw, 4);
  }
  const int64_t chunks = (T + chunk - 1) / chunk;
  RmsBwdArgs a{reinterpret_cast<const uint16_t*>(dy.first), reinterpret_cast<const uint16_t*>(h.first),
               reinterpret_cast<const uint16_t*>(dres.first), reinterpret_cast<uint16_t*>(dh.first),
               reinterpret_cast<const void*>(w), reinterpret_cast<const float*>(rstd),
               reinterpret_cast<float*>(partials), dy.second, h.second, dres.second, dh.second, T, (int)d, (int)chunk,
               w_f32 ? 1 : 0};
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  for_slices(d, [&](auto ns) {
    constexpr int NS = decltype(ns)::value;
    if (dw) hipLaunchKernelGGL((k_rmsnorm_bwd<NS, true>), dim3((unsigned)chunks), dim3(kThreads), 0, st, a);
    else hipLaunchKernelGGL((k_rmsnorm_bwd<NS, false>), dim3((unsigned)chunks), dim3(kThreads), 0, st, a);
  });
  if (dw)
    hipLaunchKernelGGL(k_rmsnorm_dw, dim3((unsigned)((d + kRmsDwCols - 1) / kRmsDwCols)), dim3(kThreads), 0, st,
                       reinterpret_cast<const float*>(partials), reinterpret_cast<float*>(dw), chunks, (int)d);
  CCMPI_HIP_CHECK(hipGetLastError());
}

}  // namespace

void register_rmsnorm_ops(pybind11::module_& m) {
  namespace py = pybind11;
  m.attr("RMS_NORM_MAX_D") = kRmsMaxD;
  m.def("rms_norm_row_chunk", [](int64_t T, int64_t d) { return rms_norm_row_chunk(T, d); }, py::arg("T"), py::arg("d"));
  m.def("rms_norm_fwd", &rms_norm_fwd,
        "h = bf16(x + residual) (or x: residual = h = (0, 0)), rstd [T] fp32 = 1 / sqrt(mean h^2 + eps), y = bf16(h rstd w); "
        "x, residual, h, y: (address, row stride in elements) of [T, d] bf16 views, h may be x or residual; w [d] bf16 "
        "or (w_f32) fp32",
        py::arg("x"), py::arg("residual"), py::arg("h"), py::arg("y"), py::arg("w"), py::arg("w_f32"), py::arg("rstd"),
        py::arg("T"), py::arg("d"), py::arg("eps"), py::arg("stream"), py::call_guard<py::gil_scoped_release>());
  m.def("rms_norm_bwd", &rms_norm_bwd,
        "dh = bf16(rstd (dy w - n mean(dy w n)) + dres), n = h rstd (dres = (0, 0): none; dh may be dy or dres); dw != 0: "
        "dw [d] fp32 = sum_t dy n through partials [ceil(T / chunk), d] fp32, chunk = rms_norm_row_chunk(T, d)",
        py::arg("dy"), py::arg("h"), py::arg("dres"), py::arg("dh"), py::arg("w"), py::arg("w_f32"), py::arg("rstd"),
        py::arg("partials"), py::arg("dw"), py::arg("T"), py::arg("d"), py::arg("chunk"), py::arg("stream"),
        py::call_guard<py::gil_scoped_release>());
}

}  // namespace dev
}  // namespace ccmpi
