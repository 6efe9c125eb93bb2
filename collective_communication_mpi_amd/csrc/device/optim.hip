// AdamW with on-device gradient-norm clipping over flat gradient buckets (ops.optim_sqsum,
// ops.optim_clip, ops.optim_adamw_update; parallel.AdamW).  A bucket is a flat gradient buffer
// g [n] (bf16 or fp32) cut into S segments, one per parameter, in bucket order:
//   seg_off [S + 1] int64   element offsets, seg_off[0] = 0, seg_off[S] = n, strictly increasing
//   seg_ptr [S] int64       address of the parameter's contiguous storage (dtype of g)
//   seg_flags [S] int32     bit 0: weight decay applies; bit 1: counted in the "sharded" norm sum
// all three on the device.  The optimizer state (p32 for bf16, m, v: fp32 [n]) is indexed like g.
//
// Slots.  Work is cut into slots of kOptimChunk = 2048 elements that start at each segment's first
// element: segment i owns the slots from seg_off[i] / 2048 + i on, there are n / 2048 + S slots, a
// workgroup bisects seg_off for its slot, and a slot past its segment's end is spare.  A workgroup
// walks the slots wg, wg + grid, ...  Thread t of 256 owns elements [8 t, 8 t + 8) of the slot:
// 16-byte accesses where the segment's offset is a multiple of 8 and (for the parameter) its base is
// 16-byte aligned, scalar accesses otherwise and for a segment's tail.  Both forms visit the same
// elements in the same thread in the same order, so the bits do not depend on the form.  All index
// arithmetic is 64-bit.
//
//   k_optim_sqsum  partials[slot] = sum of squares of the slot's gradients, fp32: the thread's 8
//                  elements in order, the xor butterfly of its wave, (w0 + w1) + (w2 + w3): 16
//                  dependent additions.  A spare slot writes +0.
//   k_optim_sums   ONE workgroup of 1024 adds a bucket's partials in fp64: thread t the slots t,
//                  t + 1024, ... in that order, into the sharded or the replicated sum by the
//                  segment's flag, then a fixed tree over the threads.  No atomics.
//   k_optim_clip   ONE thread adds the buckets' sharded sums in bucket order, the replicated sums
//                  in bucket order, the two totals; norm = float(sqrt(total)), coef = min(1,
//                  max_norm / (norm + 1e-6)) in fp32 (a NaN stays a NaN); clip = (norm, coef).
//   k_optim_adamw  per element, every operation rounded once (no contraction):
//                    g' = g coef (no clip tensor: g' = g)
//                    m' = (b1 m) + (omb1 g');  v' = (b2 v) + ((omb2 g') g')
//                    p1 = decays ? p decay : p
//                    p' = p1 - lr ((m' / bc1) / (sqrt(v' / bc2) + eps))
//                  (lr, bc1, bc2, decay) = sched [4] and coef = clip[1] are read from the device, so
//                  a captured graph stays valid across steps.  bf16: p is p32, the parameter gets
//                  bf16_rne(p'); fp32: the parameter is its own master.  Every element is read and
//                  written by the same thread; gradients are never written.
#include <hip/hip_runtime.h>
#include <pybind11/pybind11.h>

#include <cmath>
#include <stdexcept>
#include <string>

#include "common.hpp"
#include "ops.hpp"
#include "optim.hpp"

namespace ccmpi {
namespace dev {

namespace {

constexpr int kThreads = kOptimThreads;
constexpr int kWaves = kThreads / 64;
static_assert(kWaves == 4, "the wave tree below is (w0 + w1) + (w2 + w3)");
static_assert(kOptimChunk == 8 * kThreads, "a thread owns 8 consecutive elements of a slot");

struct Slot {
  int seg;
  int64_t begin;  // the segment's first element
  int64_t b, e;   // the slot's elements [b, e) of the bucket; e <= b: spare
};

// the segment that owns `slot`: the last i with seg_off[i] / chunk + i <= slot; `lo` is a segment
// known not to lie behind it (0: none)
__device__ __forceinline__ int find_seg(const int64_t* __restrict__ seg_off, int lo, int S, int64_t slot) {
  int hi = S;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (seg_off[mid] / kOptimChunk + mid <= slot) lo = mid;
    else hi = mid;
  }
  return lo;
}

__device__ __forceinline__ int64_t clamp64(int64_t x, int64_t lo, int64_t hi) { return x < lo ? lo : (x > hi ? hi : x); }

// offsets are clamped into [0, n]: whatever the table holds, g and the state are read inside [0, n)
__device__ __forceinline__ Slot find_slot(const int64_t* __restrict__ seg_off, int S, int64_t n, int64_t slot) {
  Slot s;
  s.seg = find_seg(seg_off, 0, S, slot);
  s.begin = clamp64(seg_off[s.seg], 0, n);
  const int64_t end = clamp64(seg_off[s.seg + 1], s.begin, n);
  const int64_t tile = slot - (s.begin / kOptimChunk + s.seg);
  s.b = s.begin + (tile < 0 ? 0 : tile) * kOptimChunk;
  s.e = tile < 0 ? s.b : (s.b + kOptimChunk < end ? s.b + kOptimChunk : end);
  return s;
}

__device__ __forceinline__ void unpack8(u32x4 v, float (&x)[8]) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    x[2 * i] = bf16_lo(v[i]);
    x[2 * i + 1] = bf16_hi(v[i]);
  }
}

__device__ __forceinline__ void load8(const float* p, float (&x)[8]) {
  const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
  x[0] = a.x, x[1] = a.y, x[2] = a.z, x[3] = a.w, x[4] = b.x, x[5] = b.y, x[6] = b.z, x[7] = b.w;
}

__device__ __forceinline__ void store8(float* p, const float (&x)[8]) {
  *reinterpret_cast<float4*>(p) = make_float4(x[0], x[1], x[2], x[3]);
  *reinterpret_cast<float4*>(p + 4) = make_float4(x[4], x[5], x[6], x[7]);
}

template <bool F32>
__device__ __forceinline__ float load_grad(const void* g, int64_t i) {
  if constexpr (F32) return static_cast<const float*>(g)[i];
  else return __uint_as_float((uint32_t) static_cast<const uint16_t*>(g)[i] << 16);
}

// gradients [e0, e0 + 8) of the bucket as fp32; vec: one (bf16) or two (fp32) 16-byte loads
template <bool F32>
__device__ __forceinline__ void load_grad8(const void* g, int64_t e0, float (&x)[8]) {
  if constexpr (F32) load8(static_cast<const float*>(g) + e0, x);
  else unpack8(*reinterpret_cast<const u32x4*>(static_cast<const uint16_t*>(g) + e0), x);
}

// The workgroup's sum of one value per thread: a fixed butterfly, then a fixed tree over the waves.
// ONE barrier: the caller alternates the LDS slot between consecutive sums (see rmsnorm.hip).
__device__ __forceinline__ float block_sum(float v, float* s_red) {
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) v = __fadd_rn(v, __shfl_xor(v, s, 64));
  if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
  __syncthreads();
  return __fadd_rn(__fadd_rn(s_red[0], s_red[1]), __fadd_rn(s_red[2], s_red[3]));
}

template <bool F32>
__global__ void __launch_bounds__(kThreads) k_optim_sqsum(const void* __restrict__ g, const int64_t* __restrict__ seg_off,
                                                          int S, int64_t n, int64_t slots, float* __restrict__ partials) {
  __shared__ float s_red[2 * kWaves];
  int it = 0;
  for (int64_t slot = blockIdx.x; slot < slots; slot += gridDim.x, ++it) {
    const Slot s = find_slot(seg_off, S, n, slot);
    const int64_t e0 = s.b + 8 * (int64_t)threadIdx.x;
    float acc = 0.0f;
    if (e0 < s.e) {
      if ((s.begin & 7) == 0 && e0 + 8 <= s.e) {
        float x[8];
        load_grad8<F32>(g, e0, x);
#pragma unroll
        for (int j = 0; j < 8; ++j) acc = __fmaf_rn(x[j], x[j], acc);
      } else {
        for (int j = 0; j < 8 && e0 + j < s.e; ++j) {
          const float x = load_grad<F32>(g, e0 + j);
          acc = __fmaf_rn(x, x, acc);
        }
      }
    }
    const float total = block_sum(acc, s_red + (it & 1) * kWaves);
    if (threadIdx.x == 0) partials[slot] = total;
  }
}

// ONE workgroup of kOptimSumThreads.  Thread t adds the slots t, t + 1024, ... in that order (eight
// loads in flight); a thread's slots ascend, so it keeps its segment and the first slot of the
// next one in registers and bisects again, from there on, only when a slot has left the segment.
__global__ void __launch_bounds__(kOptimSumThreads) k_optim_sums(const float* __restrict__ partials,
                                                                 const int64_t* __restrict__ seg_off,
                                                                 const int32_t* __restrict__ seg_flags, int S,
                                                                 int64_t slots, double* __restrict__ out_sharded,
                                                                 double* __restrict__ out_replicated) {
  __shared__ double s_sh[kOptimSumThreads], s_rep[kOptimSumThreads];
  constexpr int kBatch = 8;
  double sh = 0.0, rep = 0.0;
  int seg = 0;
  int64_t next_first = 0;  // the first slot of segment seg + 1; 0: nothing located yet
  bool sharded = false;
  for (int64_t base = threadIdx.x; base < slots; base += (int64_t)kBatch * kOptimSumThreads) {
    float x[kBatch];
#pragma unroll
    for (int j = 0; j < kBatch; ++j) {
      const int64_t slot = base + (int64_t)j * kOptimSumThreads;
      x[j] = slot < slots ? partials[slot] : 0.0f;
    }
#pragma unroll
    for (int j = 0; j < kBatch; ++j) {  // slot order
      const int64_t slot = base + (int64_t)j * kOptimSumThreads;
      if (slot >= slots) break;
      if (slot >= next_first) {
        seg = find_seg(seg_off, seg, S, slot);
        next_first = seg + 1 < S ? seg_off[seg + 1] / kOptimChunk + seg + 1 : slots;
        sharded = (seg_flags[seg] & kOptimSharded) != 0;
      }
      if (sharded) sh = __dadd_rn(sh, (double)x[j]);
      else rep = __dadd_rn(rep, (double)x[j]);
    }
  }
  s_sh[threadIdx.x] = sh;
  s_rep[threadIdx.x] = rep;
  __syncthreads();
  for (int s = kOptimSumThreads / 2; s >= 1; s >>= 1) {  // a fixed tree
    if ((int)threadIdx.x < s) {
      s_sh[threadIdx.x] = __dadd_rn(s_sh[threadIdx.x], s_sh[threadIdx.x + s]);
      s_rep[threadIdx.x] = __dadd_rn(s_rep[threadIdx.x], s_rep[threadIdx.x + s]);
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    *out_sharded = s_sh[0];
    *out_replicated = s_rep[0];
  }
}

__global__ void __launch_bounds__(64) k_optim_clip(const double* __restrict__ sharded,
                                                   const double* __restrict__ replicated, int nb, float max_norm,
                                                   float* __restrict__ clip) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double a = 0.0, b = 0.0;
  for (int i = 0; i < nb; ++i) a = __dadd_rn(a, sharded[i]);  // bucket order
  for (int i = 0; i < nb; ++i) b = __dadd_rn(b, replicated[i]);
  const float norm = (float)sqrt(__dadd_rn(a, b));
  const float c = __fdiv_rn(max_norm, __fadd_rn(norm, 1e-6f));
  clip[0] = norm;
  clip[1] = c > 1.0f ? 1.0f : c;  // a NaN stays a NaN
}

struct AdamArgs {
  const void* g;
  const int64_t* seg_off;
  const int64_t* seg_ptr;
  const int32_t* seg_flags;
  float* p32;  // bf16 form only
  float* m;
  float* v;
  const float* clip;   // nullptr: no clipping
  const float* sched;  // (lr, bc1, bc2, decay)
  int64_t n, slots;
  int S;
  float b1, omb1, b2, omb2, eps;
};

struct AdamConsts {
  float coef, lr, bc1, bc2, decay, b1, omb1, b2, omb2, eps;
  bool clip;
};

// The IEEE square root, rounded to nearest even (__fsqrt_rn is the hardware's approximation here).
__device__ __forceinline__ float sqrt_rn(float x) { return __builtin_sqrtf(x); }

// one element: (g, p, m, v) -> (p', m', v'), every operation rounded once.  __fmul_rn and its kin
// are plain operators that carry the translation unit's contraction mode, and p1 - lr * u would
// become one FMA: the operators are written out here, with contraction off, and the division and
// the square root are the correctly rounded ones
__device__ __forceinline__ void adamw_one(const AdamConsts& c, bool decays, float g, float& p, float& m, float& v) {
#pragma clang fp contract(off)
  if (c.clip) g = g * c.coef;
  const float m1 = c.b1 * m, m2 = c.omb1 * g;
  m = m1 + m2;
  const float v1 = c.b2 * v, v2 = c.omb2 * g, v3 = v2 * g;
  v = v1 + v3;
  const float p1 = decays ? p * c.decay : p;
  const float mh = m / c.bc1, vh = v / c.bc2;
  const float den = sqrt_rn(vh) + c.eps;
  const float u = mh / den;
  const float lu = c.lr * u;
  p = p1 - lu;
}

template <bool F32>
__global__ void __launch_bounds__(kThreads) k_optim_adamw(const AdamArgs a) {
  AdamConsts c;
  c.clip = a.clip != nullptr;
  c.coef = c.clip ? a.clip[1] : 1.0f;
  c.lr = a.sched[0], c.bc1 = a.sched[1], c.bc2 = a.sched[2], c.decay = a.sched[3];
  c.b1 = a.b1, c.omb1 = a.omb1, c.b2 = a.b2, c.omb2 = a.omb2, c.eps = a.eps;
  for (int64_t slot = blockIdx.x; slot < a.slots; slot += gridDim.x) {
    const Slot s = find_slot(a.seg_off, a.S, a.n, slot);
    const int64_t e0 = s.b + 8 * (int64_t)threadIdx.x;
    if (e0 >= s.e) continue;
    const uint64_t base = (uint64_t)a.seg_ptr[s.seg];
    const bool decays = (a.seg_flags[s.seg] & kOptimDecay) != 0;
    const int64_t q0 = e0 - s.begin;  // the element's index in its parameter
    if ((s.begin & 7) == 0 && (base & 15) == 0 && e0 + 8 <= s.e) {
      float g[8], p[8], m[8], v[8];
      load_grad8<F32>(a.g, e0, g);
      if constexpr (F32) load8(reinterpret_cast<const float*>(base) + q0, p);
      else load8(a.p32 + e0, p);
      load8(a.m + e0, m);
      load8(a.v + e0, v);
#pragma unroll
      for (int j = 0; j < 8; ++j) adamw_one(c, decays, g[j], p[j], m[j], v[j]);
      store8(a.m + e0, m);
      store8(a.v + e0, v);
      if constexpr (F32) {
        store8(reinterpret_cast<float*>(base) + q0, p);
      } else {
        store8(a.p32 + e0, p);
        u32x4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = pk_bf16(p[2 * j], p[2 * j + 1]);
        *reinterpret_cast<u32x4*>(reinterpret_cast<uint16_t*>(base) + q0) = o;
      }
    } else {
      for (int j = 0; j < 8 && e0 + j < s.e; ++j) {
        const int64_t i = e0 + j;
        float p, m = a.m[i], v = a.v[i];
        if constexpr (F32) p = reinterpret_cast<const float*>(base)[q0 + j];
        else p = a.p32[i];
        adamw_one(c, decays, load_grad<F32>(a.g, i), p, m, v);
        a.m[i] = m;
        a.v[i] = v;
        if constexpr (F32) {
          reinterpret_cast<float*>(base)[q0 + j] = p;
        } else {
          a.p32[i] = p;
          reinterpret_cast<uint16_t*>(base)[q0 + j] = (uint16_t)f32_to_bf16_bits(p);
        }
      }
    }
  }
}

[[noreturn]] void refuse(const std::string& what) { throw std::invalid_argument("optim: " + what); }

void check_buffer(const char* what, uint64_t ptr, int align) {
  if (ptr == 0 || ptr % align) refuse(std::string(what) + " must be " + std::to_string(align) + "-byte aligned");
}

int64_t check_table(int64_t n, int64_t S, uint64_t seg_off, int64_t max_grid) {
  if (n < 1 || n > kOptimMaxElems) refuse("1 <= n <= 2^40 required");
  if (S < 1 || S > kOptimMaxSegs || S > n) refuse("1 <= S <= min(n, 2^24) required");
  if (max_grid < 0 || max_grid > kOptimMaxGrid) refuse("max_grid must be in [0, 4096]");
  check_buffer("seg_off", seg_off, 8);
  return optim_slots(n, S);
}

unsigned grid_for(int64_t slots, int64_t max_grid) {
  const int64_t cap = max_grid ? max_grid : kOptimMaxGrid;
  return (unsigned)(slots < cap ? slots : cap);
}

void optim_sqsum(uint64_t g, bool f32, uint64_t seg_off, uint64_t seg_flags, int64_t S, int64_t n, uint64_t partials,
                 uint64_t out_sharded, uint64_t out_replicated, int64_t max_grid, uint64_t stream) {
  const int64_t slots = check_table(n, S, seg_off, max_grid);
  check_buffer("the gradient bucket", g, 16);
  check_buffer("seg_flags", seg_flags, 4);
  check_buffer("partials", partials, 4);
  if ((out_sharded == 0) != (out_replicated == 0)) refuse("the two sums come together");
  if (out_sharded) {
    check_buffer("sums", out_sharded, 8);
    check_buffer("sums", out_replicated, 8);
  }
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const auto* off = reinterpret_cast<const int64_t*>(seg_off);
  auto* part = reinterpret_cast<float*>(partials);
  if (f32)
    hipLaunchKernelGGL(k_optim_sqsum<true>, dim3(grid_for(slots, max_grid)), dim3(kThreads), 0, st,
                       reinterpret_cast<const void*>(g), off, (int)S, n, slots, part);
  else
    hipLaunchKernelGGL(k_optim_sqsum<false>, dim3(grid_for(slots, max_grid)), dim3(kThreads), 0, st,
                       reinterpret_cast<const void*>(g), off, (int)S, n, slots, part);
  if (out_sharded)
    hipLaunchKernelGGL(k_optim_sums, dim3(1), dim3(kOptimSumThreads), 0, st, part, off,
                       reinterpret_cast<const int32_t*>(seg_flags), (int)S, slots,
                       reinterpret_cast<double*>(out_sharded), reinterpret_cast<double*>(out_replicated));
  CCMPI_HIP_CHECK(hipGetLastError());
}

void optim_clip(uint64_t sharded, uint64_t replicated, int64_t nb, double max_norm, uint64_t clip, uint64_t stream) {
  if (nb < 1 || nb > (1 << 20)) refuse("1 <= buckets <= 2^20 required");
  if (!(max_norm > 0.0) || !std::isfinite(max_norm) || !((float)max_norm > 0.0f) || !std::isfinite((float)max_norm))
    refuse("max_norm must be a positive finite float");
  check_buffer("sums", sharded, 8);
  check_buffer("sums", replicated, 8);
  check_buffer("clip", clip, 4);
  hipLaunchKernelGGL(k_optim_clip, dim3(1), dim3(64), 0, reinterpret_cast<hipStream_t>(stream),
                     reinterpret_cast<const double*>(sharded), reinterpret_cast<const double*>(replicated), (int)nb,
                     (float)max_norm, reinterpret_cast<float*>(clip));
  CCMPI_HIP_CHECK(hipGetLastError());
}

void optim_adamw(uint64_t g, bool f32, uint64_t seg_off, uint64_t seg_ptr, uint64_t seg_flags, int64_t S, int64_t n,
                 uint64_t p32, uint64_t m, uint64_t v, uint64_t clip, uint64_t sched, double b1, double b2, double eps,
                 int64_t max_grid, uint64_t stream) {
  const int64_t slots = check_table(n, S, seg_off, max_grid);
  check_buffer("the gradient bucket", g, 16);
  check_buffer("seg_ptr", seg_ptr, 8);
  check_buffer("seg_flags", seg_flags, 4);
  if (f32) {
    if (p32) refuse("an fp32 bucket has no p32: the parameter is its own master");
  } else {
    check_buffer("p32", p32, 16);
  }
  check_buffer("m", m, 16);
  check_buffer("v", v, 16);
  if (clip) check_buffer("clip", clip, 4);
  check_buffer("sched", sched, 4);
  if (!(b1 >= 0.0 && b1 < 1.0) || !(b2 >= 0.0 && b2 < 1.0)) refuse("betas must be in [0, 1)");
  if (!(eps >= 0.0) || !std::isfinite(eps)) refuse("eps must be a non-negative finite float");
  AdamArgs a{reinterpret_cast<const void*>(g),
             reinterpret_cast<const int64_t*>(seg_off),
             reinterpret_cast<const int64_t*>(seg_ptr),
             reinterpret_cast<const int32_t*>(seg_flags),
             reinterpret_cast<float*>(p32),
             reinterpret_cast<float*>(m),
             reinterpret_cast<float*>(v),
             reinterpret_cast<const float*>(clip),
             reinterpret_cast<const float*>(sched),
             n,
             slots,
             (int)S,
             (float)b1,
             (float)(1.0 - b1),
             (float)b2,
             (float)(1.0 - b2),
             (float)eps};
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (f32) hipLaunchKernelGGL(k_optim_adamw<true>, dim3(grid_for(slots, max_grid)), dim3(kThreads), 0, st, a);
  else hipLaunchKernelGGL(k_optim_adamw<false>, dim3(grid_for(slots, max_grid)), dim3(kThreads), 0, st, a);
  CCMPI_HIP_CHECK(hipGetLastError());
}

}  // namespace

void register_optim_ops(pybind11::module_& m) {
  namespace py = pybind11;
  m.attr("OPTIM_CHUNK") = kOptimChunk;
  m.attr("OPTIM_MAX_GRID") = kOptimMaxGrid;
  m.def("optim_sqsum", &optim_sqsum,
        "partials[slot] fp32 = sum of squares of the slot's gradients (g [n] bf16, or fp32 with f32), then the bucket's "
        "partials added in fp64 into *out_sharded (segments with flag bit 1) and *out_replicated (the rest; both 0: the "
        "first level alone); "
        "partials holds n / OPTIM_CHUNK + S floats",
        py::arg("g"), py::arg("f32"), py::arg("seg_off"), py::arg("seg_flags"), py::arg("S"), py::arg("n"),
        py::arg("partials"), py::arg("out_sharded"), py::arg("out_replicated"), py::arg("max_grid"), py::arg("stream"),
        py::call_guard<py::gil_scoped_release>());
  m.def("optim_clip", &optim_clip,
        "clip [2] fp32 = (norm, coef): norm = float(sqrt(sum sharded[0:nb] + sum replicated[0:nb])) (fp64 sums, bucket "
        "order), coef = min(1, max_norm / (norm + 1e-6)) in fp32",
        py::arg("sharded"), py::arg("replicated"), py::arg("nb"), py::arg("max_norm"), py::arg("clip"),
        py::arg("stream"), py::call_guard<py::gil_scoped_release>());
  m.def("optim_adamw", &optim_adamw,
        "one AdamW step of a bucket: fp32 m, v (and p32 for a bf16 bucket) [n] indexed like g; (lr, bc1, bc2, decay) = "
        "sched [4] fp32 and coef = clip[1] (clip = 0: no clipping) are read on the device; the parameters at seg_ptr "
        "are written in the bucket's dtype",
        py::arg("g"), py::arg("f32"), py::arg("seg_off"), py::arg("seg_ptr"), py::arg("seg_flags"), py::arg("S"),
        py::arg("n"), py::arg("p32"), py::arg("m"), py::arg("v"), py::arg("clip"), py::arg("sched"), py::arg("b1"),
        py::arg("b2"), py::arg("eps"), py::arg("max_grid"), py::arg("stream"),
        py::call_guard<py::gil_scoped_release>());
}

}  // namespace dev
}  // namespace ccmpi
