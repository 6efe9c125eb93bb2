// Router logits of the routed MoE layer on the matrix cores (parallel/moe.py RoutedMoE,
// router_logits="mfma"): logits[T, E] = x[T, D] . router[E, D]^T with x in bf16 and the fp32
// router held as three bf16 planes, router = p0 + p1 + p2 exactly
//   p0 = bf16(r), p1 = bf16(r - p0), p2 = bf16(r - p0 - p1)       (fp32 subtractions, RNE),
// so every product x * plane is exact in the MFMA's fp32 accumulator and only the accumulation
// rounds, as in an fp32 GEMM.
//
//   k_split_bf16x3       fp32 [R, C] -> bf16 planes.  Every output "slot" takes one plane
//                        (slot s: plane (map >> 2 s) & 3) and is a [R, C] matrix (or its
//                        transpose [C, R]) at dst + s * slot_stride with row stride ld, so
//                        slots can be stacked ([planes, R, C]) or laid side by side along the
//                        fast axis ([R, n * C'], what the backward's GEMMs reduce over).  The
//                        fast axis is written up to fpad >= its extent, zeros past the data.
//                        64 x 64 tiles through LDS, so both forms read and write coalesced.
//   k_moe_router_logits  the 128 x 128 tile of gemm_tile128.hpp (fragment layout, nt_mfmas,
//                        direct epilogue) with one A tile and THREE B tiles per K step: the
//                        workgroup stages x's 128 x 64 tile once and runs it against the tiles
//                        of planes 2, 1, 0 (small terms first) into the same accumulators.
//                        A stage is (128 + 3 * 128) rows of 128 B = 64 KiB, two stages 128 KiB
//                        of the CU's 160 KiB.  When T is too small for a workgroup per CU the
//                        row tile shrinks to 64 or 32 rows (same columns, same order of sums).
//                        GLDS: staged by LDS-DMA (D % 64 == 0); otherwise through registers
//                        with a zero-filled K tail (any D % 8 == 0).
//                        No split-K and no atomics: one output element is accumulated over the
//                        K tiles in order, planes 2, 1, 0 inside a tile, whatever T and the
//                        row's position are, so a token's logits do not depend on its batch.
#include <pybind11/pybind11.h>

#include <climits>

#include "common.hpp"
#include "gemm_common.hpp"
#include "gemm_tile128.hpp"
#include "moe_gate.hpp"
#include "ops.hpp"

namespace ccmpi {
namespace dev {

namespace {

using namespace gemm;

constexpr int kPlanes = 3;
constexpr int kPlaneTile = BN * kRowBytes;
// one stage: RM rows of x + three plane tiles of BN rows, 128 B each
constexpr int stage_bytes(int rm) { return (rm + kPlanes * BN) * kRowBytes; }
static_assert(2 * stage_bytes(BM) <= 160 * 1024, "two stages must fit the LDS");

// ---------------------------------------------------------------------------
// split
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_split_bf16x3(const float* __restrict__ w, uint16_t* __restrict__ dst,
                                                      int64_t R, int C, int nslots, uint32_t map,
                                                      int64_t slot_stride, int64_t ld, int64_t fpad, int transpose,
                                                      int tiles_c) {
  __shared__ float tile[64][65];
  const int64_t r0 = (int64_t)(blockIdx.x / tiles_c) * 64;
  const int c0 = (int)(blockIdx.x % tiles_c) * 64;
  const int cl = threadIdx.x & 63, rl0 = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int rl = rl0 + 4 * i;
    const int64_t r = r0 + rl;
    const int c = c0 + cl;
    tile[rl][cl] = (r < R && c < C) ? w[r * C + c] : 0.0f;
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int sl = rl0 + 4 * i;
    float v;
    int64_t slow, fast;
    bool ok;
    if (transpose) {
      v = tile[cl][sl];
      slow = c0 + sl;
      fast = r0 + cl;
      ok = slow < C && fast < fpad;
    } else {
      v = tile[sl][cl];
      slow = r0 + sl;
      fast = c0 + cl;
      ok = slow < R && fast < fpad;
    }
    if (!ok) continue;
    // every subtraction is exact in fp32, every rounding to nearest even
    const uint32_t h0 = f32_to_bf16_bits(v);
    const float r1 = v - bf2f((uint16_t)h0);
    const uint32_t h1 = f32_to_bf16_bits(r1);
    const float r2 = r1 - bf2f((uint16_t)h1);
    const uint32_t h2 = f32_to_bf16_bits(r2);
    uint16_t* o = dst + slow * ld + fast;
    for (int s = 0; s < nslots; ++s) {
      const uint32_t p = (map >> (2 * s)) & 3u;
      o[s * slot_stride] = (uint16_t)(p == 0 ? h0 : p == 1 ? h1 : h2);
    }
  }
}

void split_bf16x3(uint64_t src, uint64_t dst, int64_t R, int64_t C, int nslots, uint32_t map, int64_t slot_stride,
                  int64_t ld, int64_t fpad, bool transpose, uint64_t stream) {
  if (R < 0 || C < 0 || C > INT_MAX - 64 || R > (int64_t)INT_MAX - 64)
    throw std::invalid_argument("split_bf16x3: 0 <= R, C < 2^31 - 64 required");
  if (nslots < 1 || nslots > 4) throw std::invalid_argument("split_bf16x3: 1 to 4 output slots");
  for (int s = 0; s < nslots; ++s)
    if (((map >> (2 * s)) & 3u) >= (uint32_t)kPlanes) throw std::invalid_argument("split_bf16x3: planes are 0, 1, 2");
  const int64_t F = transpose ? R : C;
  if (fpad < F || ld < fpad || slot_stride < 0) throw std::invalid_argument("split_bf16x3: fpad >= extent and ld >= fpad");
  if (src % 4 || dst % 2) throw std::invalid_argument("split_bf16x3: misaligned buffers");
  if (R == 0 || C == 0) return;
  // tiles of the input; the padded axis is the output's fast one
  const int64_t tiles_r = ((transpose ? fpad : R) + 63) / 64, tiles_c = ((transpose ? C : fpad) + 63) / 64;
  if (tiles_r * tiles_c > INT_MAX) throw std::invalid_argument("split_bf16x3: too many tiles");
  hipLaunchKernelGGL(k_split_bf16x3, dim3((unsigned)(tiles_r * tiles_c)), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), reinterpret_cast<const float*>(src),
                     reinterpret_cast<uint16_t*>(dst), R, (int)C, nslots, map, slot_stride, ld, fpad, transpose ? 1 : 0,
                     (int)tiles_c);
  CCMPI_HIP_CHECK(hipGetLastError());
}

// ---------------------------------------------------------------------------
// logits
// ---------------------------------------------------------------------------
struct RouterArgs {
  const uint16_t* X;  // [T, D] bf16, row stride ldx
  const uint16_t* P;  // [3, E, D] bf16, contiguous
  float* out;         // [T, E] fp32, contiguous
  int T, E, D, ldx;
};

// MI: 16-row MFMA fragments per wave, i.e. a row tile of RM = 32 MI rows (128, 64 or 32) against
// the same 128 columns; the waves stay 2 x 2, each MI x 4 MFMA tiles.  A smaller row tile only
// changes which workgroup computes an element, never the order it is accumulated in, so the
// launcher may pick it from T (to fill the CUs) without the logits depending on T.
// FAST: the direct vector epilogue (E % 8 == 0, 16-B aligned out); otherwise per element.
template <int MI, bool GLDS, bool FAST>
__global__ void __launch_bounds__(NT) k_moe_router_logits(RouterArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int RM = 32 * MI, kStage = stage_bytes(RM), kAB = RM * kRowBytes;
  const int tiles_n = (a.E + BN - 1) / BN, tiles_m = (int)(((int64_t)a.T + RM - 1) / RM);
  // the column tiles of one row tile get consecutive logical ids on one XCD: x's tile is
  // fetched into that XCD's L2 once
  const int wg = xcd_remap(blockIdx.x, tiles_n * tiles_m);
  const int bm = (wg / tiles_n) * RM, bn = (wg % tiles_n) * BN;
  const int t = threadIdx.x, lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int wm = (wave >> 1) * (16 * MI), wn = (wave & 1) * 64;
  // everything below is relative to the tile: row and column counts stay small ints for any T
  const int rows = min(a.T - bm, RM), cols = min(a.E - bn, BN);  // valid rows of x / of a plane (>= 1)
  const uint16_t* X = a.X + (size_t)bm * a.ldx;
  const uint16_t* P = a.P + (size_t)bn * a.D;
  const size_t pstride = (size_t)a.E * a.D;
  const int nk = (a.D + BK - 1) / BK;

  // the fragment layout of the shared tile; the plane tiles start RM (not BM) rows in
  NtFragOff fo = nt_frag_off(wm, wn, lane);
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) fo.b[ks] -= (BM - RM) * kRowBytes;
  floatx4 acc[MI][4];
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = floatx4{0.f, 0.f, 0.f, 0.f};
  auto stage = [&](int buf) { return smem + buf * kStage; };
  // nt_mfmas<true> (operands swapped for the direct epilogue) over MI row fragments
  auto mfmas = [&](const bf16x8 (&af)[2][MI], const bf16x8 (&bf)[2][4]) {
    if constexpr (MI == 4) {
      nt_mfmas<true>(af, bf, acc);
    } else {
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bf[ks][j], af[ks][i], acc[i][j], 0, 0, 0);
    }
  };
  auto compute = [&](const bf16x8 (&af)[2][MI], const bf16x8 (&bf)[kPlanes][2][4]) {
    mfmas(af, bf[2]);  // small terms first
    mfmas(af, bf[1]);
    mfmas(af, bf[0]);
  };
  auto read_frags = [&](const unsigned char* sb, bf16x8 (&af)[2][MI], bf16x8 (&bf)[kPlanes][2][4]) {
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
#pragma unroll
      for (int i = 0; i < MI; ++i) af[ks][i] = *reinterpret_cast<const bf16x8*>(sb + fo.a[ks] + i * 16 * kRowBytes);
#pragma unroll
      for (int p = 0; p < kPlanes; ++p)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          bf[p][ks][j] = *reinterpret_cast<const bf16x8*>(sb + fo.b[ks] + p * kPlaneTile + j * 16 * kRowBytes);
    }
  };

  if constexpr (GLDS) {
    // nt_loop_glds with three B tiles: rows past the valid ones re-read the last valid row
    const int lrow = lane >> 3, pchunk = lane & 7;
    auto issue = [&](int k0, int buf) {
      unsigned char* sb = stage(buf);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int q = wave * 4 + i;  // 1 KiB LDS chunk = rows q * 8 .. + 7 of a plane tile
        const int r = q * 8 + lrow;
        const int c = pchunk ^ (r & 7);
        const int gb = min(pair_perm(r), cols - 1);
#pragma unroll
        for (int p = 0; p < kPlanes; ++p)
          __builtin_amdgcn_global_load_lds((const void*)(P + p * pstride + (size_t)gb * a.D + k0 + c * 8),
                                           (__attribute__((address_space(3))) void*)(sb + kAB + p * kPlaneTile + q * 1024),
                                           16, 0, 0);
      }
#pragma unroll
      for (int i = 0; i < MI; ++i) {
        const int q = wave * MI + i;  // the x tile has 4 MI chunks
        const int r = q * 8 + lrow;
        const int c = pchunk ^ (r & 7);
        const int ga = min(r, rows - 1);
        __builtin_amdgcn_global_load_lds((const void*)(X + (size_t)ga * a.ldx + k0 + c * 8),
                                         (__attribute__((address_space(3))) void*)(sb + q * 1024), 16, 0, 0);
      }
    };
    issue(0, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    for (int kt = 0; kt < nk; ++kt) {
      const int cur = kt & 1;
      // all fragment reads before the next tile's DMA is issued (see nt_loop_glds)
      bf16x8 af[2][MI], bf[kPlanes][2][4];
      read_frags(stage(cur), af, bf);
      if (kt + 1 < nk) issue((kt + 1) * BK, cur ^ 1);
      __builtin_amdgcn_s_setprio(1);
      compute(af, bf);
      __builtin_amdgcn_s_setprio(0);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
    }
  } else {
    // nt_loop_regs with three B tiles: rows past the valid ones and the K tail are zero
    uint4 ra[MI], rb[kPlanes][4];
    const int srow = t >> 3, schunk = t & 7;
    auto gload = [&](int k0) {
      const int gk = k0 + schunk * 8;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int r = srow + 32 * i;
        const int gn = pair_perm(r);
        if (i < MI)
          ra[i < MI ? i : 0] = (r < rows && gk < a.D) ? *reinterpret_cast<const uint4*>(X + (size_t)r * a.ldx + gk)
                                                      : uint4{0, 0, 0, 0};
#pragma unroll
        for (int p = 0; p < kPlanes; ++p)
          rb[p][i] = (gn < cols && gk < a.D) ? *reinterpret_cast<const uint4*>(P + p * pstride + (size_t)gn * a.D + gk)
                                             : uint4{0, 0, 0, 0};
      }
    };
    auto swrite = [&](int buf) {
      unsigned char* sb = stage(buf);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int r = srow + 32 * i;
        const int off = r * kRowBytes + ((schunk ^ (r & 7)) << 4);
        if (i < MI) *reinterpret_cast<uint4*>(sb + off) = ra[i < MI ? i : 0];
#pragma unroll
        for (int p = 0; p < kPlanes; ++p) *reinterpret_cast<uint4*>(sb + kAB + p * kPlaneTile + off) = rb[p][i];
      }
    };
    gload(0);
    swrite(0);
    __syncthreads();
    for (int kt = 0; kt < nk; ++kt) {
      const int cur = kt & 1;
      if (kt + 1 < nk) gload((kt + 1) * BK);
      bf16x8 af[2][MI], bf[kPlanes][2][4];
      read_frags(stage(cur), af, bf);
      compute(af, bf);
      if (kt + 1 < nk) swrite(cur ^ 1);
      __syncthreads();
    }
  }

  float* C = a.out + (size_t)bm * a.E + bn;
  if constexpr (FAST && MI == 4) {
    store_direct_fast<false>(TileDst{C, a.E, rows, cols, 1.0f, nullptr, 0}, acc, wm, wn, lane);
  } else {
    // store_direct_fast's layout over MI row fragments: acc[i][2 p + h][r] is
    // C[wm + 16 i + (lane & 15)][wn + 32 p + 8 (lane >> 4) + 4 h + r]
    const int c = lane & 15, gq = lane >> 4;
#pragma unroll
    for (int i = 0; i < MI; ++i) {
      const int row = wm + 16 * i + c;
#pragma unroll
      for (int p = 0; p < 2; ++p) {
        const int col = wn + 32 * p + 8 * gq;
        if (row >= rows || col >= cols) continue;
        float* dst = C + (size_t)row * a.E + col;
        if constexpr (FAST) {
          reinterpret_cast<float4*>(dst)[0] = make_float4(acc[i][2 * p][0], acc[i][2 * p][1], acc[i][2 * p][2], acc[i][2 * p][3]);
          reinterpret_cast<float4*>(dst)[1] =
              make_float4(acc[i][2 * p + 1][0], acc[i][2 * p + 1][1], acc[i][2 * p + 1][2], acc[i][2 * p + 1][3]);
        } else {
#pragma unroll
          for (int e = 0; e < 8; ++e)
            if (col + e < cols) dst[e] = acc[i][2 * p + (e >> 2)][e & 3];
        }
      }
    }
  }
}

template <int MI>
void launch_router_logits(const RouterArgs& a, bool glds, bool fast, hipStream_t st) {
  constexpr int kLds = 2 * stage_bytes(32 * MI);
  static const bool attr = [] {
    bool ok = true;
    for (const void* f : {reinterpret_cast<const void*>(k_moe_router_logits<MI, true, true>),
                          reinterpret_cast<const void*>(k_moe_router_logits<MI, true, false>),
                          reinterpret_cast<const void*>(k_moe_router_logits<MI, false, true>),
                          reinterpret_cast<const void*>(k_moe_router_logits<MI, false, false>)})
      ok = ok && hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, kLds) == hipSuccess;
    return ok;
  }();
  if (!attr) throw std::runtime_error("moe_router_logits: cannot reserve the kernel's LDS");
  const int64_t nwg = (((int64_t)a.T + 32 * MI - 1) / (32 * MI)) * ((a.E + BN - 1) / BN);
  const dim3 grid((unsigned)nwg), block(NT);
  if (glds && fast) hipLaunchKernelGGL((k_moe_router_logits<MI, true, true>), grid, block, kLds, st, a);
  else if (glds) hipLaunchKernelGGL((k_moe_router_logits<MI, true, false>), grid, block, kLds, st, a);
  else if (fast) hipLaunchKernelGGL((k_moe_router_logits<MI, false, true>), grid, block, kLds, st, a);
  else hipLaunchKernelGGL((k_moe_router_logits<MI, false, false>), grid, block, kLds, st, a);
}

// row_tile: 128, 64 or 32 rows per workgroup; 0: the largest that gives every CU a workgroup
// (32 when none does).  The result does not depend on it.
void moe_router_logits_fwd(uint64_t x, uint64_t planes, uint64_t out, int64_t T, int E, int D, int64_t ldx,
                           int row_tile, uint64_t stream) {
  if (E < 1 || E > kGateMaxExperts) throw std::invalid_argument("moe_router_logits: 1 <= E <= 256 required");
  if (T < 0 || T > INT_MAX - kGateChunk) throw std::invalid_argument("moe_router_logits: 0 <= T < 2^31 - 64 required");
  if (D < 8 || D % 8 || ldx % 8 || ldx < D || ldx > INT_MAX)
    throw std::invalid_argument("moe_router_logits: D and x's row stride must be positive multiples of 8");
  if (x % 16 || planes % 16 || out % 4) throw std::invalid_argument("moe_router_logits: misaligned buffers");
  if (row_tile != 0 && row_tile != 32 && row_tile != 64 && row_tile != 128)
    throw std::invalid_argument("moe_router_logits: row_tile must be 0 (auto), 32, 64 or 128");
  if (T == 0) return;
  if (row_tile == 0) {
    const int64_t tiles_n = (E + BN - 1) / BN, cus = device_cus();
    row_tile = ((T + 127) / 128) * tiles_n >= cus ? 128 : ((T + 63) / 64) * tiles_n >= cus ? 64 : 32;
  }
  RouterArgs a{reinterpret_cast<const uint16_t*>(x), reinterpret_cast<const uint16_t*>(planes),
               reinterpret_cast<float*>(out), (int)T, E, D, (int)ldx};
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const bool glds = D % BK == 0, fast = E % 8 == 0 && out % 16 == 0;
  if (row_tile == 128) launch_router_logits<4>(a, glds, fast, st);
  else if (row_tile == 64) launch_router_logits<2>(a, glds, fast, st);
  else launch_router_logits<1>(a, glds, fast, st);
  CCMPI_HIP_CHECK(hipGetLastError());
}

}  // namespace

void register_moe_router_ops(pybind11::module_& m) {
  m.def("split_bf16x3", &split_bf16x3,
        "fp32 src [R, C] -> bf16 planes (p0 = bf16(w), p1 = bf16(w - p0), p2 = bf16(w - p0 - p1)): slot s, plane "
        "(map >> 2 s) & 3, is [R, C] (transpose: [C, R]) at dst + s * slot_stride, row stride ld; the fast axis is "
        "written up to fpad, zeros past the data",
        pybind11::arg("src"), pybind11::arg("dst"), pybind11::arg("R"), pybind11::arg("C"), pybind11::arg("nslots"),
        pybind11::arg("map"), pybind11::arg("slot_stride"), pybind11::arg("ld"), pybind11::arg("fpad"),
        pybind11::arg("transpose"), pybind11::arg("stream"), pybind11::call_guard<pybind11::gil_scoped_release>());
  m.def("moe_router_logits_fwd", &moe_router_logits_fwd,
        "out [T, E] fp32 = x [T, D] bf16 (row stride ldx) . (p0 + p1 + p2)^T, planes [3, E, D] bf16; row_tile: rows per "
        "workgroup (0 auto, 32, 64, 128), which the result does not depend on",
        pybind11::arg("x"), pybind11::arg("planes"), pybind11::arg("out"), pybind11::arg("T"), pybind11::arg("E"),
        pybind11::arg("D"), pybind11::arg("ldx"), pybind11::arg("row_tile"), pybind11::arg("stream"),
        pybind11::call_guard<pybind11::gil_scoped_release>());
}

}  // namespace dev
}  // namespace ccmpi
