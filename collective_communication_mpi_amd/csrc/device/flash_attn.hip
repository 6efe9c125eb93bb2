// Causal / full GQA self-attention at real sequence lengths, forward and backward, on
// v_mfma_f32_16x16x32_bf16 (ops.flash_attention; the "flash" attention of parallel/llama_dp.py).
//
// q [B, S, Hq, D], k / v [B, S, Hkv, D] bf16 are read as strided views (unit stride on D, every
// other stride a multiple of 8 elements, 16-B aligned base): the projections' outputs as they
// are, or column slices of a fused QKV buffer.  Query head h reads kv head h / (Hq / Hkv); K and
// V are never expanded.  D in {64, 128}, any S >= 1 (ragged tails are masked), fp32 accumulation.
//
// Every 16x16 product keeps the QUERY or the KEY on the MFMA column (lane & 15 = c, g = lane >> 4;
// an accumulator register r holds row 4g + r), so softmax statistics are per-lane scalars and an
// accumulator tile is the next product's B operand with no lane movement: two accumulator tiles
// packed to bf16 are the 8 k-elements of a lane, in the order k-slot (g, j) <-> row
// 16 (j >> 2) + 4g + (j & 3) of the 32 rows.  The other operand of such a product is a TRANSPOSED
// LDS image whose columns are stored in that same order (perm64), so it is one 16-B read.
//
//   k_flash_fwd      workgroup = kFlashBQ query rows of one (batch, query head), 4 waves x
//                    kFlashQT 16-row tiles, Q in registers.  Per step of kFlashBK keys: K row-major
//                    and V transposed in LDS (next step's global loads in flight behind the
//                    MFMAs), S^T = K Q^T, online softmax in the exp2 domain, O^T += V^T P^T.
//                    Under the causal mask the key loop ends at the diagonal block (tiles above
//                    it are skipped, not masked) and a wave skips steps wholly above its rows.
//                    out [B, S, Hq, D] bf16 contiguous, lse [B, Hq, S] fp32 (natural log).
//                    The running maximum is applied at every step: there is NO deferred-rescale
//                    threshold, so there is no second build to compare against.
//   k_flash_delta    delta[b, h, s] = sum_d dout * out, from the stored bf16 out, as the diagonal of an
//                    MFMA product so that it is summed in the order of dP.
//   k_flash_bwd_dkv  workgroup = kFlashBK keys of one (batch, kv head), 16 keys per wave, K and V
//                    in registers, dK^T and dV^T in accumulators.  It sweeps its Hq / Hkv query
//                    heads in order and, inside each, the kFlashBwdQ-row query steps in order:
//                    S = Q K^T and dP = dO V^T with the key on the lane, P = exp2(c S - lse),
//                    dS = P (dP - delta), dV^T += dO^T P, dK^T += Q^T dS.
//   k_flash_bwd_dq   workgroup = kFlashBQ query rows of one (batch, query head); per key step
//                    S^T, dP^T with the query on the lane, dQ^T += K^T dS^T.
// Chunk form (ops.flash_attention_chunk, the kernels of parallel/context_parallel.py): the same four
// kernels with separate lengths Sq (rows of q, dout, out, dq, lse, delta) and Sk (rows of k, v, dk,
// dv) and the position q_pos0 >= 0 of query row 0; causal: key j is visible to row i iff
// j <= q_pos0 + i, so key 0 is visible to every row and no row is ever fully masked.  Every skip
// rule moves with the offset: the forward / dQ key loop ends at min(Sk, q_pos0 + q0 + kFlashBQ), a
// wave skips steps above q_pos0 + its last row, the dK/dV kernel starts at query step
// max(0, key0 - q_pos0) / kFlashBwdQ, and a key block no query of the chunk sees has zero steps and
// stores exact zeros (a reduce-scatter sums it).  A row's sums run over the same key steps in the
// same order whichever chunk holds it and a wholly masked step is an exact no-op (alpha = 1,
// p = 0), so out, lse and dq of a chunk are bitwise the full call's rows.  SEG: the key axis of
// k / v / dk / dv is cut into segments of L keys (Sk % L == 0), key j at (j / L) * seg + (j % L) * s,
// each tensor with strides of its own: [n, B, L, Hkv, D], the layout an all-gather of per-rank
// shards produces.  The map is applied per key row in every fetch and store, so a tile may
// straddle segments; keys >= Sk and whatever lies between segments are never touched.  Self-attention
// is the kSelf instantiation of the same kernels, where Sq = Sk and q_pos0 = 0 are compile-time facts:
// the code, the speed and the bits it always had.
//
// P is recomputed in both backward kernels (seven products per tile pair instead of five): no
// atomics, no hand-off between workgroups, every sum has one owner and a fixed order, so all
// five outputs are bitwise reproducible.  Only plain vector stores write global memory.
#include <hip/hip_runtime.h>
#include <pybind11/pybind11.h>

#include <cmath>
#include <stdexcept>
#include <string>

#include "common.hpp"
#include "flash_attn.hpp"
#include "ops.hpp"

namespace ccmpi {
namespace dev {

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f4 __attribute__((ext_vector_type(4)));

constexpr float kLog2e = 1.4426950408889634f;
constexpr float kLn2 = 0.6931471805599453f;

struct Strides {
  int64_t b, s, h;  // elements
};

struct FwdArgs {
  const uint16_t *q, *k, *v;
  uint16_t* out;
  float* lse;
  Strides sq, sk, sv;
  int Sq, Hq, Hkv;
  float scale_log2;
  // the chunk form's own arguments follow those of self-attention, whose layout is unchanged
  int Sk, q_pos0, L;
  int64_t kseg, vseg;  // segment strides of k / v (kSegmented only)
};

struct BwdArgs {
  const uint16_t *q, *k, *v, *dout;
  const float *lse, *delta;
  uint16_t *dq, *dk, *dv;
  Strides sq, sk, sv, sdo;
  int Sq, Hq, Hkv;
  float scale, scale_log2;
  // the chunk form's own arguments follow those of self-attention, whose layout is unchanged
  int Sk, q_pos0, L;
  Strides sdk, sdv;
  int64_t kseg, vseg, dkseg, dvseg;  // segment strides of k / v / dk / dv (kSegmented only)
};

// Instantiations of every kernel.  kSelf is self-attention as it always was: one length (Sk = Sq),
// q_pos0 = 0 and contiguous dk / dv are compile-time facts there, so it keeps its code and its
// speed; kChunk reads Sq, Sk and q_pos0 from the arguments and writes dk / dv through their
// strides; kSegmented adds the segmented key axis.
constexpr int kSelf = 0, kChunk = 1, kSegmented = 2;

// Element offset of key row `key` on the key axis of k / v / dk / dv.  SEG: the axis is cut into
// segments of L keys, `seg` elements apart (the rank-major layout of an all-gather); otherwise
// one run of stride s.  Applied per key row, so a tile may straddle segments.
template <bool SEG>
__device__ __forceinline__ int64_t key_off(int key, int L, int64_t seg, int64_t s) {
  if (!SEG) return (int64_t)key * s;
  const int n = key / L;
  return (int64_t)n * seg + (int64_t)(key - n * L) * s;
}

__device__ __forceinline__ f4 mma32(bf16x8 a, bf16x8 b, f4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ uint4 ld_g16(const uint16_t* p, bool ok) {
  return ok ? *reinterpret_cast<const uint4*>(p) : uint4{0, 0, 0, 0};
}
__device__ __forceinline__ bf16x8 as_frag(uint4 x) { return __builtin_bit_cast(bf16x8, x); }
__device__ __forceinline__ bf16x8 ld_lds16(const uint16_t* p) { return *reinterpret_cast<const bf16x8*>(p); }
__device__ __forceinline__ void st_lds16(uint16_t* p, uint4 x) { *reinterpret_cast<uint4*>(p) = x; }
// two accumulator tiles (rows 4g + r of row tiles 0 and 1) -> the 8 k-elements of this lane
__device__ __forceinline__ bf16x8 pack8(f4 lo, f4 hi) {
  const uint4 u{pk_bf16(lo[0], lo[1]), pk_bf16(lo[2], lo[3]), pk_bf16(hi[0], hi[1]), pk_bf16(hi[2], hi[3])};
  return __builtin_bit_cast(bf16x8, u);
}
// column of row `r` (< 64) in a transposed LDS image: k-slot order of pack8 within each 32 rows
__device__ __forceinline__ int perm64(int r) {
  return (r & 32) | (((r >> 2) & 3) << 3) | (((r >> 4) & 1) << 2) | (r & 3);
}
// 8 consecutive columns col0.. of one row -> T[col][pos] of the transposed image
__device__ __forceinline__ void st_transposed(uint16_t* T, int ld, int col0, int pos, uint4 x) {
  const uint32_t w[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
  for (int e = 0; e < 8; ++e) T[(col0 + e) * ld + pos] = (uint16_t)(w[e >> 1] >> (16 * (e & 1)));
}
__device__ __forceinline__ float fast_exp2(float x) { return __builtin_amdgcn_exp2f(x); }
__device__ __forceinline__ void st_g8(uint16_t* p, f4 v, float mul) {
  *reinterpret_cast<uint2*>(p) = uint2{pk_bf16(v[0] * mul, v[1] * mul), pk_bf16(v[2] * mul, v[3] * mul)};
}

template <int D, bool CAUSAL, int MODE>
__global__ __launch_bounds__(kFlashThreads) void k_flash_fwd(const FwdArgs a) {
  constexpr int LDK = D + 8, LDT = kFlashBK + 8, KK = D / 32, DT = D / 16;
  constexpr int KP = kFlashBK * (D / 8) / kFlashThreads, VP = D / 32;
  __shared__ __attribute__((aligned(16))) uint16_t Ks[kFlashBK * LDK];
  __shared__ __attribute__((aligned(16))) uint16_t Vt[D * LDT];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = lane & 15, g = lane >> 4;
  const int qb = (int)(gridDim.x - 1 - blockIdx.x), h = blockIdx.y, b = blockIdx.z;  // heaviest blocks first
  constexpr bool SEG = MODE == kSegmented;
  const int hk = h / (a.Hq / a.Hkv), Sq = a.Sq, Sk = MODE ? a.Sk : Sq, p0 = MODE ? a.q_pos0 : 0;  // query row i sits at position p0 + i
  const int q0 = qb * kFlashBQ, qw = q0 + wave * (16 * kFlashQT);
  const uint16_t* qp = a.q + b * a.sq.b + h * a.sq.h;
  const uint16_t* kp = a.k + b * a.sk.b + hk * a.sk.h;
  const uint16_t* vp = a.v + b * a.sv.b + hk * a.sv.h;

  bf16x8 qf[kFlashQT][KK];
#pragma unroll
  for (int t = 0; t < kFlashQT; ++t) {
    const int qi = qw + 16 * t + c;
#pragma unroll
    for (int kk = 0; kk < KK; ++kk) qf[t][kk] = as_frag(ld_g16(qp + (int64_t)qi * a.sq.s + 32 * kk + 8 * g, qi < Sq));
  }
  f4 o[kFlashQT][DT];
  float m[kFlashQT], l[kFlashQT];
#pragma unroll
  for (int t = 0; t < kFlashQT; ++t) {
    m[t] = -INFINITY;
    l[t] = 0.f;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) o[t][dt] = f4{0.f, 0.f, 0.f, 0.f};
  }

  const int kend = CAUSAL ? min(Sk, p0 + q0 + kFlashBQ) : Sk;
  const int nt = (kend + kFlashBK - 1) / kFlashBK;
  uint4 kr[KP], vr[VP];
  auto fetch = [&](int key0) {
#pragma unroll
    for (int i = 0; i < KP; ++i) {
      const int p = tid + kFlashThreads * i, key = key0 + p / (D / 8);
      kr[i] = ld_g16(kp + key_off<SEG>(key, a.L, a.kseg, a.sk.s) + (p % (D / 8)) * 8, key < Sk);
    }
#pragma unroll
    for (int i = 0; i < VP; ++i) {
      const int key = key0 + lane;
      vr[i] = ld_g16(vp + key_off<SEG>(key, a.L, a.vseg, a.sv.s) + (wave + 4 * i) * 8, key < Sk);
    }
  };
  fetch(0);
  for (int it = 0; it < nt; ++it) {
    const int key0 = it * kFlashBK;
    __syncthreads();
#pragma unroll
    for (int i = 0; i < KP; ++i) {
      const int p = tid + kFlashThreads * i;
      st_lds16(Ks + (p / (D / 8)) * LDK + (p % (D / 8)) * 8, kr[i]);
    }
#pragma unroll
    for (int i = 0; i < VP; ++i) st_transposed(Vt, LDT, (wave + 4 * i) * 8, perm64(lane), vr[i]);
    __syncthreads();
    if (it + 1 < nt) fetch(key0 + kFlashBK);
    if (CAUSAL && key0 > p0 + qw + 16 * kFlashQT - 1) continue;  // every key above every row of this wave

    f4 s[4][kFlashQT];  // s[kt][t][r] = score of key key0 + 16 kt + 4g + r, query qw + 16 t + c
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) {
      bf16x8 ka[KK];
#pragma unroll
      for (int kk = 0; kk < KK; ++kk) ka[kk] = ld_lds16(Ks + (16 * kt + c) * LDK + 32 * kk + 8 * g);
#pragma unroll
      for (int t = 0; t < kFlashQT; ++t) {
        f4 acc{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kk = 0; kk < KK; ++kk) acc = mma32(ka[kk], qf[t][kk], acc);
        s[kt][t] = acc;
      }
    }
    const bool edge = key0 + kFlashBK > Sk || (CAUSAL && key0 + kFlashBK - 1 > p0 + qw);
#pragma unroll
    for (int t = 0; t < kFlashQT; ++t) {
      const int qi = qw + 16 * t + c;
      float mx = -INFINITY;
#pragma unroll
      for (int kt = 0; kt < 4; ++kt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float x = s[kt][t][r] * a.scale_log2;
          if (edge) {
            const int key = key0 + 16 * kt + 4 * g + r;
            if (key >= Sk || (CAUSAL && key > p0 + qi)) x = -INFINITY;
          }
          s[kt][t][r] = x;
          mx = fmaxf(mx, x);
        }
      mx = fmaxf(mx, __shfl_xor(mx, 16));
      mx = fmaxf(mx, __shfl_xor(mx, 32));
      // key 0 is visible to every row (p0 >= 0) and step 0 is never skipped, so mn is finite from step 0
      // on; a later step that is wholly masked for a row is an exact no-op (alpha = 1, p = 0)
      const float mn = fmaxf(m[t], mx);
      const float alpha = fast_exp2(m[t] - mn);
      m[t] = mn;
      float sum = 0.f;
#pragma unroll
      for (int kt = 0; kt < 4; ++kt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float p = fast_exp2(s[kt][t][r] - mn);
          s[kt][t][r] = p;
          sum += p;
        }
      l[t] = l[t] * alpha + sum;  // this lane's 16 keys of every step; the four g are added at the end
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) o[t][dt] *= alpha;
    }
#pragma unroll
    for (int cc = 0; cc < 2; ++cc) {
      bf16x8 pf[kFlashQT];
#pragma unroll
      for (int t = 0; t < kFlashQT; ++t) pf[t] = pack8(s[2 * cc][t], s[2 * cc + 1][t]);
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) {
        const bf16x8 va = ld_lds16(Vt + (16 * dt + c) * LDT + 32 * cc + 8 * g);
#pragma unroll
        for (int t = 0; t < kFlashQT; ++t) o[t][dt] = mma32(va, pf[t], o[t][dt]);
      }
    }
  }
#pragma unroll
  for (int t = 0; t < kFlashQT; ++t) {
    const int qi = qw + 16 * t + c;
    float lt = l[t] + __shfl_xor(l[t], 16);
    lt += __shfl_xor(lt, 32);
    if (qi >= Sq) continue;
    const float inv = 1.0f / lt;
    uint16_t* op = a.out + (((int64_t)b * Sq + qi) * a.Hq + h) * D + 4 * g;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) st_g8(op + 16 * dt, o[t][dt], inv);
    if (g == 0) a.lse[((int64_t)b * a.Hq + h) * Sq + qi] = (m[t] + __log2f(lt)) * kLn2;
  }
}

// delta of 16 rows per wave as the DIAGONAL of the 16x16 product dO O^T: the same MFMA chain over
// D, in the same order, as the backward kernels' dP = dO V^T.  A row that sees a single key has
// O = V there, so its dP - delta, and with it its dS, dQ and dK share, is exactly zero.
template <int D>
__global__ __launch_bounds__(kFlashThreads) void k_flash_delta(const uint16_t* dout, Strides sdo, const uint16_t* out,
                                                               float* delta, int64_t rows, int S, int Hq) {
  constexpr int KK = D / 32;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
  const int64_t row = ((int64_t)blockIdx.x * (kFlashThreads / 64) + wave) * 16 + c;  // (b * S + s) * Hq + h
  const bool ok = row < rows;
  const int h = (int)(row % Hq);
  const int64_t bs = row / Hq;
  const int s = (int)(bs % S);
  const int64_t b = bs / S;
  const uint16_t* dp = dout + b * sdo.b + s * sdo.s + h * sdo.h + 8 * g;
  const uint16_t* op = out + row * D + 8 * g;
  f4 acc{0.f, 0.f, 0.f, 0.f};  // acc[r] = dout row 4g + r . out row c
#pragma unroll
  for (int kk = 0; kk < KK; ++kk) acc = mma32(as_frag(ld_g16(dp + 32 * kk, ok)), as_frag(ld_g16(op + 32 * kk, ok)), acc);
  const int r = c & 3;
  const float d = r == 0 ? acc[0] : r == 1 ? acc[1] : r == 2 ? acc[2] : acc[3];
  if (ok && (c >> 2) == g) delta[(b * Hq + h) * S + s] = d;
}

template <int D, bool CAUSAL, int MODE>
__global__ __launch_bounds__(kFlashThreads) void k_flash_bwd_dkv(const BwdArgs a) {
  constexpr int LDK = D + 8, LDQ = kFlashBwdQ + 8, KK = D / 32, DT = D / 16, NP = D / 64;
  __shared__ __attribute__((aligned(16))) uint16_t Qs[kFlashBwdQ * LDK];
  __shared__ __attribute__((aligned(16))) uint16_t Os[kFlashBwdQ * LDK];
  __shared__ __attribute__((aligned(16))) uint16_t Qt[D * LDQ];
  __shared__ __attribute__((aligned(16))) uint16_t Ot[D * LDQ];
  __shared__ __attribute__((aligned(16))) float Ls[kFlashBwdQ];
  __shared__ __attribute__((aligned(16))) float Ds[kFlashBwdQ];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = lane & 15, g = lane >> 4;
  const int kb = blockIdx.x, hk = blockIdx.y, b = blockIdx.z;
  constexpr bool SEG = MODE == kSegmented;
  const int Sq = a.Sq, Sk = MODE ? a.Sk : Sq, p0 = MODE ? a.q_pos0 : 0, rep = a.Hq / a.Hkv;
  const int key0 = kb * kFlashBK, kw = key0 + 16 * wave, keyi = kw + c;
  const uint16_t* kp = a.k + b * a.sk.b + hk * a.sk.h + key_off<SEG>(keyi, a.L, a.kseg, a.sk.s);
  const uint16_t* vp = a.v + b * a.sv.b + hk * a.sv.h + key_off<SEG>(keyi, a.L, a.vseg, a.sv.s);
  bf16x8 kf[KK], vf[KK];
#pragma unroll
  for (int kk = 0; kk < KK; ++kk) {
    kf[kk] = as_frag(ld_g16(kp + 32 * kk + 8 * g, keyi < Sk));
    vf[kk] = as_frag(ld_g16(vp + 32 * kk + 8 * g, keyi < Sk));
  }
  f4 dk[DT], dv[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) dk[dt] = dv[dt] = f4{0.f, 0.f, 0.f, 0.f};

  // query steps wholly before the key block see none of it; a key block past every query of the
  // chunk has no step at all and stores exact zeros
  const int qs0 = CAUSAL ? (MODE ? max(0, key0 - p0) : key0) / kFlashBwdQ : 0;
  const int nqs = (Sq + kFlashBwdQ - 1) / kFlashBwdQ - qs0, nq = MODE ? max(0, nqs) : nqs;
  const int steps = rep * nq;  // query heads in order, query steps in order inside each
  const int row = tid & 31, cb = tid >> 5;
  uint4 qr[NP], dr[NP];
  float lv = 0.f, dl = 0.f;
  auto fetch = [&](int i) {
    const int h = hk * rep + i / nq, qi = (qs0 + i % nq) * kFlashBwdQ + row;
    const bool ok = qi < Sq;
    const uint16_t* qp = a.q + b * a.sq.b + h * a.sq.h + (int64_t)qi * a.sq.s;
    const uint16_t* dp = a.dout + b * a.sdo.b + h * a.sdo.h + (int64_t)qi * a.sdo.s;
#pragma unroll
    for (int j = 0; j < NP; ++j) {
      qr[j] = ld_g16(qp + (cb + 8 * j) * 8, ok);
      dr[j] = ld_g16(dp + (cb + 8 * j) * 8, ok);
    }
    if (tid < kFlashBwdQ) {
      const int64_t o = ((int64_t)b * a.Hq + h) * Sq + qi;
      lv = ok ? a.lse[o] * kLog2e : 0.f;
      dl = ok ? a.delta[o] : 0.f;
    }
  };
  if (steps > 0) fetch(0);
  for (int i = 0; i < steps; ++i) {
    const int qbase = (qs0 + i % nq) * kFlashBwdQ;
    __syncthreads();
#pragma unroll
    for (int j = 0; j < NP; ++j) {
      const int col = (cb + 8 * j) * 8;
      st_lds16(Qs + row * LDK + col, qr[j]);
      st_lds16(Os + row * LDK + col, dr[j]);
      st_transposed(Qt, LDQ, col, perm64(row), qr[j]);
      st_transposed(Ot, LDQ, col, perm64(row), dr[j]);
    }
    if (tid < kFlashBwdQ) {
      Ls[row] = lv;
      Ds[row] = dl;
    }
    __syncthreads();
    if (i + 1 < steps) fetch(i + 1);
    if (CAUSAL && p0 + qbase + kFlashBwdQ - 1 < kw) continue;  // every query of the step before every key of this wave

    f4 p[2], ds[2];  // [t][r]: query qbase + 16 t + 4g + r, key keyi
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      f4 sa{0.f, 0.f, 0.f, 0.f}, pa{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kk = 0; kk < KK; ++kk) {
        sa = mma32(ld_lds16(Qs + (16 * t + c) * LDK + 32 * kk + 8 * g), kf[kk], sa);
        pa = mma32(ld_lds16(Os + (16 * t + c) * LDK + 32 * kk + 8 * g), vf[kk], pa);
      }
      const f4 l4 = *reinterpret_cast<const f4*>(Ls + 16 * t + 4 * g);
      const f4 d4 = *reinterpret_cast<const f4*>(Ds + 16 * t + 4 * g);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int qi = qbase + 16 * t + 4 * g + r;
        const bool dead = qi >= Sq || keyi >= Sk || (CAUSAL && keyi > p0 + qi);
        const float pv = dead ? 0.f : fast_exp2(sa[r] * a.scale_log2 - l4[r]);
        p[t][r] = pv;
        ds[t][r] = pv * (pa[r] - d4[r]);
      }
    }
    const bf16x8 pf = pack8(p[0], p[1]), dsf = pack8(ds[0], ds[1]);
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) {
      dv[dt] = mma32(ld_lds16(Ot + (16 * dt + c) * LDQ + 8 * g), pf, dv[dt]);
      dk[dt] = mma32(ld_lds16(Qt + (16 * dt + c) * LDQ + 8 * g), dsf, dk[dt]);
    }
  }
  if (keyi < Sk) {
    // self-attention: dk / dv are contiguous [B, S, Hkv, D]
    const int64_t o = MODE ? 0 : (((int64_t)b * Sk + keyi) * a.Hkv + hk) * D;
    uint16_t* dkp = a.dk + (MODE ? b * a.sdk.b + hk * a.sdk.h + key_off<SEG>(keyi, a.L, a.dkseg, a.sdk.s) : o) + 4 * g;
    uint16_t* dvp = a.dv + (MODE ? b * a.sdv.b + hk * a.sdv.h + key_off<SEG>(keyi, a.L, a.dvseg, a.sdv.s) : o) + 4 * g;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) {
      st_g8(dkp + 16 * dt, dk[dt], a.scale);
      st_g8(dvp + 16 * dt, dv[dt], 1.0f);
    }
  }
}

template <int D, bool CAUSAL, int MODE>
__global__ __launch_bounds__(kFlashThreads) void k_flash_bwd_dq(const BwdArgs a) {
  constexpr int LDK = D + 8, LDT = kFlashBK + 8, KK = D / 32, DT = D / 16, VP = D / 32;
  __shared__ __attribute__((aligned(16))) uint16_t Ks[kFlashBK * LDK];
  __shared__ __attribute__((aligned(16))) uint16_t Vs[kFlashBK * LDK];
  __shared__ __attribute__((aligned(16))) uint16_t Kt[D * LDT];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = lane & 15, g = lane >> 4;
  const int qb = (int)(gridDim.x - 1 - blockIdx.x), h = blockIdx.y, b = blockIdx.z;
  constexpr bool SEG = MODE == kSegmented;
  const int hk = h / (a.Hq / a.Hkv), Sq = a.Sq, Sk = MODE ? a.Sk : Sq, p0 = MODE ? a.q_pos0 : 0;  // query row i sits at position p0 + i
  const int q0 = qb * kFlashBQ, qw = q0 + wave * (16 * kFlashQT);
  const uint16_t* qp = a.q + b * a.sq.b + h * a.sq.h;
  const uint16_t* dop = a.dout + b * a.sdo.b + h * a.sdo.h;
  const uint16_t* kp = a.k + b * a.sk.b + hk * a.sk.h;
  const uint16_t* vp = a.v + b * a.sv.b + hk * a.sv.h;

  bf16x8 qf[kFlashQT][KK], dof[kFlashQT][KK];
  float lse2[kFlashQT], dl[kFlashQT];
  f4 dq[kFlashQT][DT];
#pragma unroll
  for (int t = 0; t < kFlashQT; ++t) {
    const int qi = qw + 16 * t + c;
    const bool ok = qi < Sq;
#pragma unroll
    for (int kk = 0; kk < KK; ++kk) {
      qf[t][kk] = as_frag(ld_g16(qp + (int64_t)qi * a.sq.s + 32 * kk + 8 * g, ok));
      dof[t][kk] = as_frag(ld_g16(dop + (int64_t)qi * a.sdo.s + 32 * kk + 8 * g, ok));
    }
    const int64_t o = ((int64_t)b * a.Hq + h) * Sq + qi;
    lse2[t] = ok ? a.lse[o] * kLog2e : 0.f;
    dl[t] = ok ? a.delta[o] : 0.f;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) dq[t][dt] = f4{0.f, 0.f, 0.f, 0.f};
  }

  const int kend = CAUSAL ? min(Sk, p0 + q0 + kFlashBQ) : Sk;
  const int nt = (kend + kFlashBK - 1) / kFlashBK;
  uint4 kr[VP], vr[VP];
  auto fetch = [&](int key0) {
    const int key = key0 + lane;
    const int64_t kof = key_off<SEG>(key, a.L, a.kseg, a.sk.s), vof = key_off<SEG>(key, a.L, a.vseg, a.sv.s);
#pragma unroll
    for (int i = 0; i < VP; ++i) {
      kr[i] = ld_g16(kp + kof + (wave + 4 * i) * 8, key < Sk);
      vr[i] = ld_g16(vp + vof + (wave + 4 * i) * 8, key < Sk);
    }
  };
  fetch(0);
  for (int it = 0; it < nt; ++it) {
    const int key0 = it * kFlashBK;
    __syncthreads();
#pragma unroll
    for (int i = 0; i < VP; ++i) {
      const int col = (wave + 4 * i) * 8;
      st_lds16(Ks + lane * LDK + col, kr[i]);
      st_lds16(Vs + lane * LDK + col, vr[i]);
      st_transposed(Kt, LDT, col, perm64(lane), kr[i]);
    }
    __syncthreads();
    if (it + 1 < nt) fetch(key0 + kFlashBK);
    if (CAUSAL && key0 > p0 + qw + 16 * kFlashQT - 1) continue;

#pragma unroll
    for (int cc = 0; cc < 2; ++cc) {
      f4 ds[2][kFlashQT];  // [u][t][r]: key key0 + 16 (2cc + u) + 4g + r, query qw + 16 t + c
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int kt = 2 * cc + u;
        bf16x8 ka[KK], va[KK];
#pragma unroll
        for (int kk = 0; kk < KK; ++kk) {
          ka[kk] = ld_lds16(Ks + (16 * kt + c) * LDK + 32 * kk + 8 * g);
          va[kk] = ld_lds16(Vs + (16 * kt + c) * LDK + 32 * kk + 8 * g);
        }
#pragma unroll
        for (int t = 0; t < kFlashQT; ++t) {
          const int qi = qw + 16 * t + c;
          f4 sa{0.f, 0.f, 0.f, 0.f}, pa{0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int kk = 0; kk < KK; ++kk) {
            sa = mma32(ka[kk], qf[t][kk], sa);
            pa = mma32(va[kk], dof[t][kk], pa);
          }
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int key = key0 + 16 * kt + 4 * g + r;
            const bool dead = qi >= Sq || key >= Sk || (CAUSAL && key > p0 + qi);
            const float pv = dead ? 0.f : fast_exp2(sa[r] * a.scale_log2 - lse2[t]);
            ds[u][t][r] = pv * (pa[r] - dl[t]);
          }
        }
      }
      bf16x8 dsf[kFlashQT];
#pragma unroll
      for (int t = 0; t < kFlashQT; ++t) dsf[t] = pack8(ds[0][t], ds[1][t]);
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) {
        const bf16x8 kt8 = ld_lds16(Kt + (16 * dt + c) * LDT + 32 * cc + 8 * g);
#pragma unroll
        for (int t = 0; t < kFlashQT; ++t) dq[t][dt] = mma32(kt8, dsf[t], dq[t][dt]);
      }
    }
  }
#pragma unroll
  for (int t = 0; t < kFlashQT; ++t) {
    const int qi = qw + 16 * t + c;
    if (qi >= Sq) continue;
    uint16_t* op = a.dq + (((int64_t)b * Sq + qi) * a.Hq + h) * D + 4 * g;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) st_g8(op + 16 * dt, dq[t][dt], a.scale);
  }
}

void check_view(const char* what, uint64_t p, const Strides& s) {
  if (p == 0 || p % 16) throw std::invalid_argument(std::string("flash_attention: ") + what + " must be 16-byte aligned");
  if (s.b % 8 || s.s % 8 || s.h % 8)
    throw std::invalid_argument(std::string("flash_attention: ") + what + " strides must be multiples of 8 elements");
}

void check_shape(int B, int64_t S, int Hq, int Hkv, int D) {
  if (D != 64 && D != 128) throw std::invalid_argument("flash_attention: head dim must be 64 or 128");
  if (B < 1 || B > 65535 || Hq < 1 || Hq > 65535) throw std::invalid_argument("flash_attention: 1 <= B, Hq <= 65535 required");
  if (Hkv < 1 || Hq % Hkv) throw std::invalid_argument("flash_attention: Hq must be a multiple of Hkv");
  if (S < 1 || S > (1 << 30)) throw std::invalid_argument("flash_attention: 1 <= S <= 2^30 required");
}

// The chunk form's own rules: separate lengths, the position of query row 0 and the key segments.
void check_chunk(int64_t Sq, int64_t Sk, int64_t L, int64_t q_pos0, int Hkv) {
  if (Sk < 1 || Sk > (1 << 30)) throw std::invalid_argument("flash_attention_chunk: 1 <= Sk <= 2^30 required");
  if (q_pos0 < 0 || q_pos0 + Sq > (1 << 30))
    throw std::invalid_argument("flash_attention_chunk: 0 <= q_pos0 and q_pos0 + Sq <= 2^30 required");
  if (L < 1 || Sk % L) throw std::invalid_argument("flash_attention_chunk: Sk must be a multiple of the segment length");
  if (Hkv > 65535) throw std::invalid_argument("flash_attention_chunk: Hkv <= 65535 required");
}

void check_seg(const char* what, int64_t seg) {
  if (seg % 8) throw std::invalid_argument(std::string("flash_attention_chunk: segment stride of ") + what + " must be a multiple of 8 elements");
}

template <typename F64, typename F128>
void by_dim(int D, F64&& f64, F128&& f128) {
  if (D == 64) f64(); else f128();
}

// One launcher per kernel: the self-attention entry points come here with Sq = Sk, q_pos0 = 0 and
// L = Sk (kSelf), the chunk entry points with their own values (kChunk, or kSegmented when L < Sk).
template <int MODE>
void launch_fwd(const FwdArgs& a, int B, int D, bool causal, hipStream_t st) {
  const dim3 grid((unsigned)((a.Sq + kFlashBQ - 1) / kFlashBQ), (unsigned)a.Hq, (unsigned)B), block(kFlashThreads);
  auto go = [&](auto kern) { hipLaunchKernelGGL(kern, grid, block, 0, st, a); };
  if (causal) by_dim(D, [&] { go(k_flash_fwd<64, true, MODE>); }, [&] { go(k_flash_fwd<128, true, MODE>); });
  else by_dim(D, [&] { go(k_flash_fwd<64, false, MODE>); }, [&] { go(k_flash_fwd<128, false, MODE>); });
}

template <int MODE>
void launch_bwd(const BwdArgs& a, const uint16_t* outp, float* deltap, int B, int D, bool causal, hipStream_t st) {
  const dim3 block(kFlashThreads);
  const int64_t rows = (int64_t)B * a.Sq * a.Hq;
  const int64_t dblocks = (rows + 16 * (kFlashThreads / 64) - 1) / (16 * (kFlashThreads / 64));
  if (dblocks > 0x7fffffffLL) throw std::invalid_argument("flash_attention: B * S * Hq too large");
  by_dim(D,
         [&] { hipLaunchKernelGGL(k_flash_delta<64>, dim3((unsigned)dblocks), block, 0, st, a.dout, a.sdo, outp, deltap, rows, a.Sq, a.Hq); },
         [&] { hipLaunchKernelGGL(k_flash_delta<128>, dim3((unsigned)dblocks), block, 0, st, a.dout, a.sdo, outp, deltap, rows, a.Sq, a.Hq); });

  const dim3 gkv((unsigned)((a.Sk + kFlashBK - 1) / kFlashBK), (unsigned)a.Hkv, (unsigned)B);
  auto gokv = [&](auto kern) { hipLaunchKernelGGL(kern, gkv, block, 0, st, a); };
  if (causal) by_dim(D, [&] { gokv(k_flash_bwd_dkv<64, true, MODE>); }, [&] { gokv(k_flash_bwd_dkv<128, true, MODE>); });
  else by_dim(D, [&] { gokv(k_flash_bwd_dkv<64, false, MODE>); }, [&] { gokv(k_flash_bwd_dkv<128, false, MODE>); });

  const dim3 gq((unsigned)((a.Sq + kFlashBQ - 1) / kFlashBQ), (unsigned)a.Hq, (unsigned)B);
  auto goq = [&](auto kern) { hipLaunchKernelGGL(kern, gq, block, 0, st, a); };
  if (causal) by_dim(D, [&] { goq(k_flash_bwd_dq<64, true, MODE>); }, [&] { goq(k_flash_bwd_dq<128, true, MODE>); });
  else by_dim(D, [&] { goq(k_flash_bwd_dq<64, false, MODE>); }, [&] { goq(k_flash_bwd_dq<128, false, MODE>); });
}

void fill_fwd(FwdArgs& a, uint64_t q, uint64_t k, uint64_t v, uint64_t out, uint64_t lse, int Hq, int Hkv, double scale) {
  check_view("q", q, a.sq);
  check_view("k", k, a.sk);
  check_view("v", v, a.sv);
  if (out == 0 || out % 16 || lse == 0 || lse % 4) throw std::invalid_argument("flash_attention: misaligned out / lse");
  a.q = reinterpret_cast<const uint16_t*>(q);
  a.k = reinterpret_cast<const uint16_t*>(k);
  a.v = reinterpret_cast<const uint16_t*>(v);
  a.out = reinterpret_cast<uint16_t*>(out);
  a.lse = reinterpret_cast<float*>(lse);
  a.Hq = Hq;
  a.Hkv = Hkv;
  a.scale_log2 = (float)(scale * 1.4426950408889634);
}

void fill_bwd(BwdArgs& a, uint64_t dout, uint64_t q, uint64_t k, uint64_t v, uint64_t out, uint64_t lse, uint64_t delta,
              uint64_t dq, uint64_t dk, uint64_t dv, int Hq, int Hkv, double scale) {
  check_view("q", q, a.sq);
  check_view("k", k, a.sk);
  check_view("v", v, a.sv);
  check_view("dout", dout, a.sdo);
  check_view("dk", dk, a.sdk);
  check_view("dv", dv, a.sdv);
  if (out == 0 || (out | dq | dk | dv) % 16 || dq == 0 || dk == 0 || dv == 0 || lse == 0 || delta == 0 || (lse | delta) % 4)
    throw std::invalid_argument("flash_attention: misaligned out / lse / delta / dq / dk / dv");
  a.q = reinterpret_cast<const uint16_t*>(q);
  a.k = reinterpret_cast<const uint16_t*>(k);
  a.v = reinterpret_cast<const uint16_t*>(v);
  a.dout = reinterpret_cast<const uint16_t*>(dout);
  a.lse = reinterpret_cast<const float*>(lse);
  a.delta = reinterpret_cast<const float*>(delta);
  a.dq = reinterpret_cast<uint16_t*>(dq);
  a.dk = reinterpret_cast<uint16_t*>(dk);
  a.dv = reinterpret_cast<uint16_t*>(dv);
  a.Hq = Hq;
  a.Hkv = Hkv;
  a.scale = (float)scale;
  a.scale_log2 = (float)(scale * 1.4426950408889634);
}

void flash_attn_fwd(uint64_t q, uint64_t k, uint64_t v, uint64_t out, uint64_t lse, int64_t q_sb, int64_t q_ss,
                    int64_t q_sh, int64_t k_sb, int64_t k_ss, int64_t k_sh, int64_t v_sb, int64_t v_ss, int64_t v_sh, int B,
                    int64_t S, int Hq, int Hkv, int D, bool causal, double scale, uint64_t stream) {
  check_shape(B, S, Hq, Hkv, D);
  FwdArgs a;
  a.sq = {q_sb, q_ss, q_sh};
  a.sk = {k_sb, k_ss, k_sh};
  a.sv = {v_sb, v_ss, v_sh};
  a.kseg = a.vseg = 0;
  fill_fwd(a, q, k, v, out, lse, Hq, Hkv, scale);
  a.Sq = a.Sk = a.L = (int)S;
  a.q_pos0 = 0;
  launch_fwd<kSelf>(a, B, D, causal, reinterpret_cast<hipStream_t>(stream));
  CCMPI_HIP_CHECK(hipGetLastError());
}

void flash_attn_bwd(uint64_t dout, uint64_t q, uint64_t k, uint64_t v, uint64_t out, uint64_t lse, uint64_t delta,
                    uint64_t dq, uint64_t dk, uint64_t dv, int64_t do_sb, int64_t do_ss, int64_t do_sh, int64_t q_sb,
                    int64_t q_ss, int64_t q_sh, int64_t k_sb, int64_t k_ss, int64_t k_sh, int64_t v_sb, int64_t v_ss,
                    int64_t v_sh, int B, int64_t S, int Hq, int Hkv, int D, bool causal, double scale, uint64_t stream) {
  check_shape(B, S, Hq, Hkv, D);
  BwdArgs a;
  a.sq = {q_sb, q_ss, q_sh};
  a.sk = {k_sb, k_ss, k_sh};
  a.sv = {v_sb, v_ss, v_sh};
  a.sdo = {do_sb, do_ss, do_sh};
  a.sdk = a.sdv = {S * Hkv * D, (int64_t)Hkv * D, (int64_t)D};  // contiguous [B, S, Hkv, D]
  a.kseg = a.vseg = a.dkseg = a.dvseg = 0;
  fill_bwd(a, dout, q, k, v, out, lse, delta, dq, dk, dv, Hq, Hkv, scale);
  a.Sq = a.Sk = a.L = (int)S;
  a.q_pos0 = 0;
  launch_bwd<kSelf>(a, reinterpret_cast<const uint16_t*>(out), reinterpret_cast<float*>(delta), B, D, causal,
                    reinterpret_cast<hipStream_t>(stream));
  CCMPI_HIP_CHECK(hipGetLastError());
}

// k / v strides come as (segment, batch, key, head); seg_len = Sk means one run (the segment
// stride is then unused and the kChunk instantiations run).
void flash_attn_chunk_fwd(uint64_t q, uint64_t k, uint64_t v, uint64_t out, uint64_t lse, int64_t q_sb, int64_t q_ss,
                          int64_t q_sh, int64_t k_sg, int64_t k_sb, int64_t k_ss, int64_t k_sh, int64_t v_sg, int64_t v_sb,
                          int64_t v_ss, int64_t v_sh, int B, int64_t Sq, int64_t Sk, int64_t seg_len, int64_t q_pos0, int Hq,
                          int Hkv, int D, bool causal, double scale, uint64_t stream) {
  check_shape(B, Sq, Hq, Hkv, D);
  check_chunk(Sq, Sk, seg_len, q_pos0, Hkv);
  FwdArgs a;
  a.sq = {q_sb, q_ss, q_sh};
  a.sk = {k_sb, k_ss, k_sh};
  a.sv = {v_sb, v_ss, v_sh};
  a.kseg = k_sg;
  a.vseg = v_sg;
  check_seg("k", k_sg);
  check_seg("v", v_sg);
  fill_fwd(a, q, k, v, out, lse, Hq, Hkv, scale);
  a.Sq = (int)Sq;
  a.Sk = (int)Sk;
  a.L = (int)seg_len;
  a.q_pos0 = (int)q_pos0;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (seg_len == Sk) launch_fwd<kChunk>(a, B, D, causal, st);
  else launch_fwd<kSegmented>(a, B, D, causal, st);
  CCMPI_HIP_CHECK(hipGetLastError());
}

void flash_attn_chunk_bwd(uint64_t dout, uint64_t q, uint64_t k, uint64_t v, uint64_t out, uint64_t lse, uint64_t delta,
                          uint64_t dq, uint64_t dk, uint64_t dv, int64_t do_sb, int64_t do_ss, int64_t do_sh, int64_t q_sb,
                          int64_t q_ss, int64_t q_sh, int64_t k_sg, int64_t k_sb, int64_t k_ss, int64_t k_sh, int64_t v_sg,
                          int64_t v_sb, int64_t v_ss, int64_t v_sh, int64_t dk_sg, int64_t dk_sb, int64_t dk_ss,
                          int64_t dk_sh, int64_t dv_sg, int64_t dv_sb, int64_t dv_ss, int64_t dv_sh, int B, int64_t Sq,
                          int64_t Sk, int64_t seg_len, int64_t q_pos0, int Hq, int Hkv, int D, bool causal, double scale,
                          uint64_t stream) {
  check_shape(B, Sq, Hq, Hkv, D);
  check_chunk(Sq, Sk, seg_len, q_pos0, Hkv);
  BwdArgs a;
  a.sq = {q_sb, q_ss, q_sh};
  a.sk = {k_sb, k_ss, k_sh};
  a.sv = {v_sb, v_ss, v_sh};
  a.sdo = {do_sb, do_ss, do_sh};
  a.sdk = {dk_sb, dk_ss, dk_sh};
  a.sdv = {dv_sb, dv_ss, dv_sh};
  a.kseg = k_sg;
  a.vseg = v_sg;
  a.dkseg = dk_sg;
  a.dvseg = dv_sg;
  check_seg("k", k_sg);
  check_seg("v", v_sg);
  check_seg("dk", dk_sg);
  check_seg("dv", dv_sg);
  fill_bwd(a, dout, q, k, v, out, lse, delta, dq, dk, dv, Hq, Hkv, scale);
  a.Sq = (int)Sq;
  a.Sk = (int)Sk;
  a.L = (int)seg_len;
  a.q_pos0 = (int)q_pos0;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const uint16_t* outp = reinterpret_cast<const uint16_t*>(out);
  float* deltap = reinterpret_cast<float*>(delta);
  if (seg_len == Sk) launch_bwd<kChunk>(a, outp, deltap, B, D, causal, st);
  else launch_bwd<kSegmented>(a, outp, deltap, B, D, causal, st);
  CCMPI_HIP_CHECK(hipGetLastError());
}

}  // namespace

void register_flash_attn_ops(pybind11::module_& m) {
  namespace py = pybind11;
  m.attr("FLASH_BQ") = kFlashBQ;
  m.attr("FLASH_BK") = kFlashBK;
  m.def("flash_attn_fwd", &flash_attn_fwd,
        "self-attention forward: q [B, S, Hq, D], k / v [B, S, Hkv, D] bf16 views (element strides b, s, h; unit "
        "stride on D) -> out [B, S, Hq, D] bf16 contiguous, lse [B, Hq, S] fp32",
        py::arg("q"), py::arg("k"), py::arg("v"), py::arg("out"), py::arg("lse"), py::arg("q_sb"), py::arg("q_ss"),
        py::arg("q_sh"), py::arg("k_sb"), py::arg("k_ss"), py::arg("k_sh"), py::arg("v_sb"), py::arg("v_ss"),
        py::arg("v_sh"), py::arg("B"), py::arg("S"), py::arg("Hq"), py::arg("Hkv"), py::arg("D"), py::arg("causal"),
        py::arg("scale"), py::arg("stream"), py::call_guard<py::gil_scoped_release>());
  m.def("flash_attn_bwd", &flash_attn_bwd,
        "self-attention backward: delta [B, Hq, S] fp32 workspace, dq [B, S, Hq, D], dk / dv [B, S, Hkv, D] bf16 "
        "contiguous; three launches (delta, dK/dV, dQ), no atomics",
        py::arg("dout"), py::arg("q"), py::arg("k"), py::arg("v"), py::arg("out"), py::arg("lse"), py::arg("delta"),
        py::arg("dq"), py::arg("dk"), py::arg("dv"), py::arg("do_sb"), py::arg("do_ss"), py::arg("do_sh"),
        py::arg("q_sb"), py::arg("q_ss"), py::arg("q_sh"), py::arg("k_sb"), py::arg("k_ss"), py::arg("k_sh"),
        py::arg("v_sb"), py::arg("v_ss"), py::arg("v_sh"), py::arg("B"), py::arg("S"), py::arg("Hq"), py::arg("Hkv"),
        py::arg("D"), py::arg("causal"), py::arg("scale"), py::arg("stream"), py::call_guard<py::gil_scoped_release>());
  m.def("flash_attn_chunk_fwd", &flash_attn_chunk_fwd,
        "chunk forward: q [B, Sq, Hq, D] at positions q_pos0.., k / v with Sk keys in segments of seg_len (element "
        "strides segment, b, s, h); causal: key j visible to row i iff j <= q_pos0 + i -> out [B, Sq, Hq, D], lse [B, Hq, Sq]",
        py::arg("q"), py::arg("k"), py::arg("v"), py::arg("out"), py::arg("lse"), py::arg("q_sb"), py::arg("q_ss"),
        py::arg("q_sh"), py::arg("k_sg"), py::arg("k_sb"), py::arg("k_ss"), py::arg("k_sh"), py::arg("v_sg"),
        py::arg("v_sb"), py::arg("v_ss"), py::arg("v_sh"), py::arg("B"), py::arg("Sq"), py::arg("Sk"), py::arg("seg_len"),
        py::arg("q_pos0"), py::arg("Hq"), py::arg("Hkv"), py::arg("D"), py::arg("causal"), py::arg("scale"),
        py::arg("stream"), py::call_guard<py::gil_scoped_release>());
  m.def("flash_attn_chunk_bwd", &flash_attn_chunk_bwd,
        "chunk backward: dq [B, Sq, Hq, D] contiguous; dk / dv written through their own (segment, b, s, h) strides; a "
        "key no query of the chunk sees gets exact zeros",
        py::arg("dout"), py::arg("q"), py::arg("k"), py::arg("v"), py::arg("out"), py::arg("lse"), py::arg("delta"),
        py::arg("dq"), py::arg("dk"), py::arg("dv"), py::arg("do_sb"), py::arg("do_ss"), py::arg("do_sh"),
        py::arg("q_sb"), py::arg("q_ss"), py::arg("q_sh"), py::arg("k_sg"), py::arg("k_sb"), py::arg("k_ss"),
        py::arg("k_sh"), py::arg("v_sg"), py::arg("v_sb"), py::arg("v_ss"), py::arg("v_sh"), py::arg("dk_sg"),
        py::arg("dk_sb"), py::arg("dk_ss"), py::arg("dk_sh"), py::arg("dv_sg"), py::arg("dv_sb"), py::arg("dv_ss"),
        py::arg("dv_sh"), py::arg("B"), py::arg("Sq"), py::arg("Sk"), py::arg("seg_len"), py::arg("q_pos0"),
        py::arg("Hq"), py::arg("Hkv"), py::arg("D"), py::arg("causal"), py::arg("scale"), py::arg("stream"),
        py::call_guard<py::gil_scoped_release>());
}

}  // namespace dev
}  // namespace ccmpi
