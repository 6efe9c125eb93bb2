// Grouped bf16 GEMM over the routed rows of an MoE layer: the experts of one rank
// applied to the buffer moe_dispatch fills, forward and backward, with the row
// counts read from device memory.
//
//   forward  out[r, :] = alpha * x[r, :] . w[g]^T (+ bias[g])   for the rows r of expert g
//   wgrad    dw[g]     = alpha * dy[rows of g]^T . x[rows of g]  (fp32)
//
// Expert g owns rows [off_g, off_g + c_g) of the [cap, *] buffers, off_g the prefix
// sum of c_g = max(counts[g], 0); the ranges are clamped to cap (counts that add up
// to more than cap truncate the last experts), so no row at or past cap is read or
// written, and rows at or past sum(c_g) are left untouched.
//
// Neither kernel's grid depends on the counts.  The forward launches
// (ceil(cap / 128) + G) * ceil(N / 128) workgroups, an upper bound on the
// sum_g ceil(c_g / 128) row tiles times the column tiles; every workgroup scans the
// (at most 256) counts at its top -- two block-wide prefix sums, rows then tiles --
// to find its (expert, row tile); the workgroups past the number of real tiles return.  Row
// tiles start at off_g, not at multiples of 128 of the buffer, so a tile never spans
// two experts; its last rows are masked in the store.  The weight gradient launches
// G * ceil(N / 128) * ceil(K / 128) workgroups; each walks its expert's rows in
// order (no split-K, no atomics: deterministic, independent of the other experts).
//
// The tile code is the 128x128, BK = 64 v_mfma_f32_16x16x32_bf16 tile of gemm.hip:
// LDS-DMA staging with the swapped-operand direct epilogue when K % 64 == 0, the
// register-staged loop with a zero-filled K tail otherwise (same LDS image, same
// epilogue); the weight gradient is k_gemm_tn's two-tiles-in-flight loop over buffer
// resources that span exactly the expert's rows, so rows past its end load as zero.
#include <pybind11/pybind11.h>

#include <algorithm>
#include <stdexcept>
#include <string>

#include "common.hpp"
#include "gemm_common.hpp"
#include "ops.hpp"

namespace ccmpi {
namespace dev {

namespace {
using namespace gemm;

constexpr int BM = 128, BN = 128, BK = 64, NT = 256;
constexpr int kRowBytes = BK * 2;
constexpr int kMaxGroups = 256;  // = MOE_MAX_EXPERTS (one count per thread of the scan)

struct GroupedArgs {
  const uint16_t* A;    // forward: x [cap, K]; wgrad: dy [cap, N]
  const uint16_t* B;    // forward: w [G][N][K] (strides ldb, b_stride); wgrad: x [cap, K]
  void* C;              // forward: out [cap, N]; wgrad: dw [G][N][K] fp32 (strides ldc, c_stride)
  const void* bias;     // forward: [G][N] (row stride bias_ld)
  const void* counts;   // [G] int32 / int64
  int cap, N, K, G;
  int lda, ldb, ldc, bias_ld;
  long long b_stride, c_stride;  // elements between experts
  float alpha;
  int bias_kind;        // 0 none, 1 fp32, 2 bf16
  int counts64;
};

__device__ __forceinline__ long long load_count(const GroupedArgs& a, int g) {
  if (g >= a.G) return 0;
  const long long c = a.counts64 ? reinterpret_cast<const long long*>(a.counts)[g]
                                 : (long long)reinterpret_cast<const int*>(a.counts)[g];
  return c < 0 ? 0 : (c > a.cap ? (long long)a.cap : c);  // (one expert never has more than cap rows)
}

// inclusive prefix sum over the 256 threads of the workgroup (ws: 4 LDS words)
__device__ __forceinline__ long long block_scan(long long v, long long* ws, int t) {
  const int lane = t & 63, wave = t >> 6;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const long long u = __shfl_up(v, d, 64);
    if (lane >= d) v += u;
  }
  if (lane == 63) ws[wave] = v;
  __syncthreads();
  long long add = 0;
  for (int w = 0; w < wave; ++w) add += ws[w];
  __syncthreads();
  return v + add;
}

// rows [off, end) of thread t's expert, clamped to cap
__device__ __forceinline__ void expert_rows(const GroupedArgs& a, long long* ws, int t, int& off, int& end) {
  const long long c = load_count(a, t);
  const long long incl = block_scan(c, ws, t);
  const long long cap = a.cap;
  off = (int)((incl - c) < cap ? (incl - c) : cap);
  end = (int)(incl < cap ? incl : cap);
}

// LDS row r of the B tile holds output column pair_perm(r) (gemm.hip: the pair permutation
// of the direct epilogue)
__device__ __forceinline__ int pair_perm(int r) {
  return (r & ~31) | (((r & 15) >> 2) << 3) | (((r >> 4) & 1) << 2) | (r & 3);
}

// ---------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------
template <bool GLDS, bool OUT_BF16>
__global__ void __launch_bounds__(NT) k_grouped_gemm_nt(GroupedArgs a) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[2 * (BM + BN) * kRowBytes];
  __shared__ long long ws[4];
  __shared__ int seg[4];  // expert, first row of the tile, end of the expert's rows; row tiles in all
  const int t = threadIdx.x, lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int tiles_n = (a.N + BN - 1) / BN;

  if (t == 0) seg[0] = -1;
  int off, end;
  expert_rows(a, ws, t, off, end);
  const long long nt = (end - off + BM - 1) / BM;
  const long long tincl = block_scan(nt, ws, t);
  if (t == NT - 1) seg[3] = (int)tincl;
  __syncthreads();
  // The real tiles are the first nreal workgroups, the rest return: the hardware deals
  // consecutive workgroups round-robin to the 8 XCDs, so every XCD gets the same share of
  // the real tiles whatever the counts are, and the remap over nreal (a bijection on
  // [0, nreal)) gives each XCD consecutive column tiles of the same rows (a shared A panel).
  const int nreal = __builtin_amdgcn_readfirstlane(seg[3]) * tiles_n;
  if ((int)blockIdx.x >= nreal) return;  // past the last real tile
  const int wg = xcd_remap(blockIdx.x, nreal);
  const int tile = wg / tiles_n, bn = (wg % tiles_n) * BN;
  if (tile >= tincl - nt && tile < tincl) {
    seg[0] = t;
    seg[1] = off + (int)(tile - (tincl - nt)) * BM;
    seg[2] = end;
  }
  __syncthreads();
  const int g = __builtin_amdgcn_readfirstlane(seg[0]);
  if (g < 0) return;
  const int bm = __builtin_amdgcn_readfirstlane(seg[1]), row_end = __builtin_amdgcn_readfirstlane(seg[2]);
  const uint16_t* Bg = a.B + (size_t)g * a.b_stride;

  const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64;
  auto As = [&](int buf) { return smem + buf * ((BM + BN) * kRowBytes); };
  auto Bs = [&](int buf) { return smem + buf * ((BM + BN) * kRowBytes) + BM * kRowBytes; };

  floatx4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = floatx4{0.f, 0.f, 0.f, 0.f};

  // the MFMAs of one staged K tile; operands swapped (B rows first) for the direct epilogue
  auto read_frags = [&](int cur, bf16x8 (&af)[2][4], bf16x8 (&bf)[2][4]) {
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const int chunk = ks * 4 + (lane >> 4);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int ra_ = wm + i * 16 + (lane & 15);
        af[ks][i] = *reinterpret_cast<const bf16x8*>(As(cur) + ra_ * kRowBytes + ((chunk ^ (ra_ & 7)) << 4));
        const int rb_ = wn + i * 16 + (lane & 15);
        bf[ks][i] = *reinterpret_cast<const bf16x8*>(Bs(cur) + rb_ * kRowBytes + ((chunk ^ (rb_ & 7)) << 4));
      }
    }
  };
  auto mfmas = [&](const bf16x8 (&af)[2][4], const bf16x8 (&bf)[2][4]) {
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bf[ks][j], af[ks][i], acc[i][j], 0, 0, 0);
  };

  if constexpr (GLDS) {
    // LDS-DMA staging (k_gemm_nt_glds): lane-linear LDS image, the (row & 7) chunk swizzle on
    // the source address.  Rows past the expert's end / past N re-read the last valid row
    // (their outputs are never stored), so nothing outside the expert's rows is touched.
    const int lrow = lane >> 3, pchunk = lane & 7;
    auto issue = [&](int k0, int buf) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int q = wave * 4 + i;
        const int r = q * 8 + lrow;
        const int c = pchunk ^ (r & 7);
        const int ga = min(bm + r, row_end - 1), gb = min(bn + pair_perm(r), a.N - 1);
        __builtin_amdgcn_global_load_lds((const void*)(a.A + (size_t)ga * a.lda + k0 + c * 8),
                                         (__attribute__((address_space(3))) void*)(As(buf) + q * 1024), 16, 0, 0);
        __builtin_amdgcn_global_load_lds((const void*)(Bg + (size_t)gb * a.ldb + k0 + c * 8),
                                         (__attribute__((address_space(3))) void*)(Bs(buf) + q * 1024), 16, 0, 0);
      }
    };
    const int nk = a.K / BK;
    if (nk > 0) issue(0, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    for (int kt = 0; kt < nk; ++kt) {
      const int cur = kt & 1;
      bf16x8 af[2][4], bf[2][4];
      read_frags(cur, af, bf);  // every fragment read before the next tile's DMA is issued
      if (kt + 1 < nk) issue((kt + 1) * BK, cur ^ 1);
      __builtin_amdgcn_s_setprio(1);
      mfmas(af, bf);
      __builtin_amdgcn_s_setprio(0);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
    }
  } else {
    // register staging (k_gemm_nt): rows past the expert's end, rows past N and the K tail
    // are zero-filled
    uint4 ra[4], rb[4];
    const int srow = t >> 3, schunk = t & 7;
    auto gload = [&](int k0) {
      const int gk = k0 + schunk * 8;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int r = srow + 32 * i;
        const int gm = bm + r, gn = bn + pair_perm(r);
        ra[i] = (gm < row_end && gk < a.K) ? *reinterpret_cast<const uint4*>(a.A + (size_t)gm * a.lda + gk) : uint4{0, 0, 0, 0};
        rb[i] = (gn < a.N && gk < a.K) ? *reinterpret_cast<const uint4*>(Bg + (size_t)gn * a.ldb + gk) : uint4{0, 0, 0, 0};
      }
    };
    auto swrite = [&](int buf) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int r = srow + 32 * i;
        const int o = r * kRowBytes + ((schunk ^ (r & 7)) << 4);
        *reinterpret_cast<uint4*>(As(buf) + o) = ra[i];
        *reinterpret_cast<uint4*>(Bs(buf) + o) = rb[i];
      }
    };
    const int nk = (a.K + BK - 1) / BK;
    if (nk > 0) {
      gload(0);
      swrite(0);
    }
    __syncthreads();
    for (int kt = 0; kt < nk; ++kt) {
      const int cur = kt & 1;
      if (kt + 1 < nk) gload((kt + 1) * BK);
      bf16x8 af[2][4], bf[2][4];
      read_frags(cur, af, bf);
      mfmas(af, bf);
      if (kt + 1 < nk) swrite(cur ^ 1);
      __syncthreads();
    }
  }

  // direct epilogue: acc[i][2p + h][r] = C[bm + wm + 16i + (lane & 15)][bn + wn + 32p + 8 (lane >> 4) + 4h + r],
  // eight consecutive columns of one row per lane and pair; rows past the expert's end are masked
  const int c = lane & 15, gq = lane >> 4;
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const int col = bn + wn + 32 * p + 8 * gq;
    float bias[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) bias[e] = 0.f;
    if (a.bias_kind == 1 && col < a.N) {
      const float* b = reinterpret_cast<const float*>(a.bias) + (size_t)g * a.bias_ld + col;
#pragma unroll
      for (int e = 0; e < 8; ++e) bias[e] = b[e];
    } else if (a.bias_kind == 2 && col < a.N) {
      const uint16_t* b = reinterpret_cast<const uint16_t*>(a.bias) + (size_t)g * a.bias_ld + col;
#pragma unroll
      for (int e = 0; e < 8; ++e) bias[e] = bf2f(b[e]);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = bm + wm + 16 * i + c;
      float v[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = a.alpha * acc[i][2 * p + (e >> 2)][e & 3] + bias[e];
      if (row < row_end && col < a.N) {
        if constexpr (OUT_BF16) {
          uint32_t w[4];
#pragma unroll
          for (int q = 0; q < 4; ++q) w[q] = pk_bf16(v[2 * q], v[2 * q + 1]);
          *reinterpret_cast<uint4*>(reinterpret_cast<uint16_t*>(a.C) + (size_t)row * a.ldc + col) =
              uint4{w[0], w[1], w[2], w[3]};
        } else {
          float4* C = reinterpret_cast<float4*>(reinterpret_cast<float*>(a.C) + (size_t)row * a.ldc + col);
          C[0] = make_float4(v[0], v[1], v[2], v[3]);
          C[1] = make_float4(v[4], v[5], v[6], v[7]);
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------
// weight gradient: dw[g][N][K] = alpha * dy[rows of g]^T . x[rows of g]
// (k_gemm_tn's PF = 2 form: 64-row tiles of both operands staged as they are, MFMA operands
// through ds_read_b64_tr_b16, two tiles in flight in two register sets)
// ---------------------------------------------------------------------------
typedef short v4s __attribute__((ext_vector_type(4)));
typedef short v8s __attribute__((ext_vector_type(8)));
constexpr int kTnRow = 288;           // bytes per LDS row (256 data + 32 pad)
constexpr int kTnTile = BK * kTnRow;  // one operand tile

__device__ __forceinline__ int tn_off(int row, int byte) { return row * kTnRow + (byte ^ (((row >> 3) & 1) << 7)); }

__global__ void __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(2))) k_grouped_gemm_tn(GroupedArgs a) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[4 * kTnTile];
  __shared__ long long ws[4];
  __shared__ int seg[2];
  const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
  // C rows = N (columns of dy), C columns = K (columns of x); the reduction runs over rows
  const int tiles_n = (a.K + BN - 1) / BN, tiles_m = (a.N + BM - 1) / BM;
  const int per = tiles_n * tiles_m;
  // expert-major grid, the XCD remap applied inside each expert: every XCD takes an equal
  // share of every expert's output tiles (consecutive ones, sharing operand panels in its
  // L2), so skewed counts load the XCDs evenly
  const int g = blockIdx.x / per;
  const int wg = xcd_remap(blockIdx.x % per, per);
  const int bm = (wg / tiles_n) * BM, bn = (wg % tiles_n) * BN;
  {
    int off, end;
    expert_rows(a, ws, t, off, end);
    if (t == g) {
      seg[0] = off;
      seg[1] = end;
    }
    __syncthreads();
  }
  const int off = __builtin_amdgcn_readfirstlane(seg[0]);
  const int rows = __builtin_amdgcn_readfirstlane(seg[1]) - off;
  const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64;
  auto As = [&](int buf) { return smem + buf * (2 * kTnTile); };
  auto Bs = [&](int buf) { return smem + buf * (2 * kTnTile) + kTnTile; };

  floatx4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = floatx4{0.f, 0.f, 0.f, 0.f};

  constexpr int PF = 2;
  uint4 ra[PF][4], rb[PF][4];
  const int schunk = t & 15, srow = t >> 4;
  const int nk = (rows + BK - 1) / BK;
  // The mask is the buffer resource: it starts at the expert's first row and ends with the
  // last element of its last row, so rows past the expert's end (the next expert's, spare
  // rows, whatever they hold) load as zero and contribute exactly nothing.  Columns past
  // N / K read the row's neighbours inside the expert, or zero on its last row; they only
  // reach outputs that are never stored.
  const uint32_t bytes_a = rows > 0 ? (uint32_t)(((size_t)(rows - 1) * a.lda + a.N) * 2) : 0u;
  const uint32_t bytes_b = rows > 0 ? (uint32_t)(((size_t)(rows - 1) * a.ldb + a.K) * 2) : 0u;
  const Rsrc rsa = make_rsrc(uniform_ptr(reinterpret_cast<char*>(const_cast<uint16_t*>(a.A + (size_t)off * a.lda))), bytes_a);
  const Rsrc rsb = make_rsrc(uniform_ptr(reinterpret_cast<char*>(const_cast<uint16_t*>(a.B + (size_t)off * a.ldb))), bytes_b);
  auto gload = [&](int s, int m0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const uint32_t m = (uint32_t)(m0 + srow + 16 * i);
      const int ca = bm + schunk * 8, cb = bn + schunk * 8;
      ra[s][i] = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(rsa.r, (m * a.lda + ca) * 2, 0, 0));
      rb[s][i] = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(rsb.r, (m * a.ldb + cb) * 2, 0, 0));
    }
  };
  auto swrite = [&](int buf, int s) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r = srow + 16 * i;
      *reinterpret_cast<uint4*>(As(buf) + tn_off(r, schunk * 16)) = ra[s][i];
      *reinterpret_cast<uint4*>(Bs(buf) + tn_off(r, schunk * 16)) = rb[s][i];
    }
  };
  const int grp = lane >> 4, q = (lane >> 2) & 3, p = lane & 3;
  const int lrow = (grp * 8 + q) * kTnRow, xsw = (grp & 1) << 7;
  const int la = lrow + ((wm * 2) ^ xsw) + 8 * p, lb = lrow + ((wn * 2) ^ xsw) + 8 * p;
  auto compute = [&](int cur) {
    const unsigned char* abase = As(cur) + la;
    const unsigned char* bbase = Bs(cur) + lb;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      bf16x8 af[4], bf[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int o = ks * 32 * kTnRow + 32 * i;
        const v4s a0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) v4s*)(abase + o));
        const v4s a1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) v4s*)(abase + o + 4 * kTnRow));
        const v4s b0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) v4s*)(bbase + o));
        const v4s b1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) v4s*)(bbase + o + 4 * kTnRow));
        af[i] = __builtin_bit_cast(bf16x8, (v8s)__builtin_shufflevector(a0, a1, 0, 1, 2, 3, 4, 5, 6, 7));
        bf[i] = __builtin_bit_cast(bf16x8, (v8s)__builtin_shufflevector(b0, b1, 0, 1, 2, 3, 4, 5, 6, 7));
      }
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bf[j], acc[i][j], 0, 0, 0);
    }
  };
  // tile j goes to register set j % 2 and LDS buffer j & 1 one step before its MFMAs
#pragma unroll
  for (int u = 0; u < PF; ++u)
    if (u < nk) gload(u, u * BK);
  if (nk > 0) swrite(0, 0);
  __syncthreads();
  if (PF < nk) gload(0, PF * BK);
  for (int kt = 0; kt < nk; kt += PF) {
#pragma unroll
    for (int u = 0; u < PF; ++u) {
      if (kt + u < nk) {
        compute(u & 1);
        if (kt + u + 1 < nk) swrite((u + 1) & 1, (u + 1) % PF);
        __syncthreads();
        if (kt + u + 1 + PF < nk) gload((u + 1) % PF, (kt + u + 1 + PF) * BK);
      }
    }
  }
  __syncthreads();
  // LDS-staged fp32 rows (the operand buffers are dead): an expert with no rows stores zeros
  float* tile = reinterpret_cast<float*>(smem);
  constexpr int TS = BN + 4;
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        tile[(wm + i * 16 + (lane >> 4) * 4 + r) * TS + wn + j * 16 + (lane & 15)] = a.alpha * acc[i][j][r];
  __syncthreads();
  float* Cg = reinterpret_cast<float*>(a.C) + (size_t)g * a.c_stride;
  for (int idx = t; idx < BM * (BN / 4); idx += NT) {
    const int rl = idx / (BN / 4), cl = (idx % (BN / 4)) * 4;
    const int row = bm + rl, col = bn + cl;
    if (row >= a.N || col >= a.K) continue;
    *reinterpret_cast<float4*>(Cg + (size_t)row * a.ldc + col) =
        make_float4(tile[rl * TS + cl], tile[rl * TS + cl + 1], tile[rl * TS + cl + 2], tile[rl * TS + cl + 3]);
  }
}

void check_common(const char* op, uint64_t A, uint64_t B, uint64_t C, uint64_t counts, int cap, int N, int K, int G,
                  int lda, int ldb) {
  const std::string who = std::string("ccmpi ") + op + ": ";
  if (G < 1 || G > kMaxGroups) throw std::invalid_argument(who + "the number of experts must be in [1, 256]");
  if (N < 8 || K < 8 || N % 8 || K % 8) throw std::invalid_argument(who + "N and K must be positive multiples of 8");
  if (lda % 8 || ldb % 8 || (A % 16) || (B % 16) || (C % 16))
    throw std::invalid_argument(who + "base pointers and row strides must be 16-B aligned");
  if (cap > 0 && (A == 0 || B == 0 || C == 0 || counts == 0)) throw std::invalid_argument(who + "null operand");
}

void grouped_gemm_nt(uint64_t X, uint64_t W, uint64_t Out, uint64_t bias, uint64_t counts, int cap, int N, int K,
                     int G, int ldx, int ldw, long long w_stride, int ldo, int bias_ld, float alpha, int bias_kind,
                     bool out_bf16, bool counts64, uint64_t stream) {
  check_common("grouped_gemm_nt", X, W, Out, counts, cap, N, K, G, ldx, ldw);
  if (w_stride % 8 || (ldo * (out_bf16 ? 2 : 4)) % 16 || bias_kind < 0 || bias_kind > 2 || (bias_kind && bias == 0))
    throw std::invalid_argument("ccmpi grouped_gemm_nt: 16-B aligned expert stride and output rows, bias kind 0..2");
  if (cap <= 0) return;
  const long long row_tiles = (cap + BM - 1) / BM + G, grid = row_tiles * ((N + BN - 1) / BN);
  if (grid >= (1ll << 31)) throw std::invalid_argument("ccmpi grouped_gemm_nt: grid too large");
  GroupedArgs a{reinterpret_cast<const uint16_t*>(X), reinterpret_cast<const uint16_t*>(W), reinterpret_cast<void*>(Out),
                reinterpret_cast<const void*>(bias), reinterpret_cast<const void*>(counts), cap, N, K, G, ldx, ldw, ldo,
                bias_ld, w_stride, 0, alpha, bias_kind, counts64 ? 1 : 0};
  auto st = reinterpret_cast<hipStream_t>(stream);
  const dim3 gr((unsigned)grid), bl(NT);
  if (K % BK == 0) {
    if (out_bf16) hipLaunchKernelGGL((k_grouped_gemm_nt<true, true>), gr, bl, 0, st, a);
    else hipLaunchKernelGGL((k_grouped_gemm_nt<true, false>), gr, bl, 0, st, a);
  } else {
    if (out_bf16) hipLaunchKernelGGL((k_grouped_gemm_nt<false, true>), gr, bl, 0, st, a);
    else hipLaunchKernelGGL((k_grouped_gemm_nt<false, false>), gr, bl, 0, st, a);
  }
  CCMPI_HIP_CHECK(hipGetLastError());
}

void grouped_gemm_tn(uint64_t dY, uint64_t X, uint64_t dW, uint64_t counts, int cap, int N, int K, int G, int lddy,
                     int ldx, int lddw, long long dw_stride, float alpha, bool counts64, uint64_t stream) {
  check_common("grouped_gemm_tn", dY, X, dW, counts, cap, N, K, G, lddy, ldx);
  if (lddw % 4 || dw_stride % 4)
    throw std::invalid_argument("ccmpi grouped_gemm_tn: 16-B aligned output rows and expert stride");
  // an expert's rows are addressed with 32-bit byte offsets from its first row
  if (cap > 0 && (size_t)cap * (size_t)std::max(lddy, ldx) * 2 >= (1ull << 31))
    throw std::invalid_argument("ccmpi grouped_gemm_tn: cap * row stride must stay below 2 GiB");
  const long long grid = (long long)G * ((N + BM - 1) / BM) * ((K + BN - 1) / BN);
  if (grid >= (1ll << 31)) throw std::invalid_argument("ccmpi grouped_gemm_tn: grid too large");
  GroupedArgs a{reinterpret_cast<const uint16_t*>(dY), reinterpret_cast<const uint16_t*>(X), reinterpret_cast<void*>(dW),
                nullptr, reinterpret_cast<const void*>(counts), cap < 0 ? 0 : cap, N, K, G, lddy, ldx, lddw, 0, 0,
                dw_stride, alpha, 0, counts64 ? 1 : 0};
  hipLaunchKernelGGL(k_grouped_gemm_tn, dim3((unsigned)grid), dim3(NT), 0, reinterpret_cast<hipStream_t>(stream), a);
  CCMPI_HIP_CHECK(hipGetLastError());
}

}  // namespace

void register_grouped_gemm_ops(pybind11::module_& m) {
  m.def("grouped_gemm_nt", &grouped_gemm_nt,
        "out[rows of g] = alpha * x[rows of g] . w[g]^T (+ bias[g]); the rows per expert read from device counts",
        pybind11::arg("x"), pybind11::arg("w"), pybind11::arg("out"), pybind11::arg("bias"), pybind11::arg("counts"),
        pybind11::arg("cap"), pybind11::arg("N"), pybind11::arg("K"), pybind11::arg("G"), pybind11::arg("ldx"),
        pybind11::arg("ldw"), pybind11::arg("w_stride"), pybind11::arg("ldo"), pybind11::arg("bias_ld"),
        pybind11::arg("alpha"), pybind11::arg("bias_kind"), pybind11::arg("out_bf16"), pybind11::arg("counts64"),
        pybind11::arg("stream"), pybind11::call_guard<pybind11::gil_scoped_release>());
  m.def("grouped_gemm_tn", &grouped_gemm_tn,
        "dw[g][N][K] = alpha * dy[rows of g]^T . x[rows of g] (fp32); the rows per expert read from device counts",
        pybind11::arg("dy"), pybind11::arg("x"), pybind11::arg("dw"), pybind11::arg("counts"), pybind11::arg("cap"),
        pybind11::arg("N"), pybind11::arg("K"), pybind11::arg("G"), pybind11::arg("lddy"), pybind11::arg("ldx"),
        pybind11::arg("lddw"), pybind11::arg("dw_stride"), pybind11::arg("alpha"), pybind11::arg("counts64"),
        pybind11::arg("stream"), pybind11::call_guard<pybind11::gil_scoped_release>());
}

}  // namespace dev
}  // namespace ccmpi
