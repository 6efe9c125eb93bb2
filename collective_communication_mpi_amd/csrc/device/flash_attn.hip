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
// dv) and the position q_pos0 >= 0 of query row 0.
//
// THE MASK has one home, struct Mask below: key j is visible to query row i iff j < Sk, i < Sq
// and, when causal, j <= q_pos0 + i; so key 0 is visible to every row and no row is ever fully
// masked.  Every skip is that rule applied to a block and is a member of Mask, used by all three
// kernels: the end of the forward / dQ key loop, the step a wave skips, the forward's edge test,
// the first query step of the dK/dV kernel.  A key block no query of the chunk sees has zero
// steps and stores exact zeros (a reduce-scatter sums it).  A row's sums run over the same key
// steps in the same order whichever chunk holds it and a wholly masked step is an exact no-op
// (alpha = 1, p = 0), so out, lse and dq of a chunk are bitwise the full call's rows.
//
// SEG: the key axis of k / v / dk / dv is cut into segments of L keys (Sk % L == 0), key j at
// (j / L) * seg + (j % L) * s, each tensor with strides of its own: [n, B, L, Hkv, D], the layout
// an all-gather of per-rank shards produces.  The map is applied per key row in every fetch and
// store, so a tile may straddle segments; keys >= Sk and whatever lies between segments are never
// touched.  Self-attention is the kSelf instantiation of the same kernels, where Sq = Sk and
// q_pos0 = 0 are compile-time facts: the code, the speed and the bits it always had.  Which
// instantiation runs is the caller's choice (the self_attention flag of the two entry points), not
// a property of the values: a chunk call with Sq = Sk and q_pos0 = 0 still runs kChunk.
//
// PACKED form (ops.flash_attention_varlen, kVarlen): q [T, Hq, D], k / v [T, Hkv, D] hold n sequences
// back to back, sequence i on rows [cu[i], cu[i + 1]) of all three; cu [n + 1] int32 is read ON THE
// DEVICE, so the host knows T and n alone (no synchronisation, capturable, and a replayed graph
// follows the contents of cu).  Inside a sequence it is self-attention (Sq = Sk = its length,
// q_pos0 = 0); no key of another sequence is visible.  The grid has T / BLK + n slots (BLK rows or
// keys per workgroup); sequence i owns those from cu[i] / BLK + i on, which never overlap since
// cu[i + 1] / BLK + 1 >= cu[i] / BLK + ceil(len_i / BLK).  A workgroup finds the sequence of its slot
// by bisection over cu (uniform loads, no LDS) and leaves before its first barrier when the slot
// is spare.  Tiles therefore start at the sequence's first row: the sums run over the same key and
// query steps in the same order as a self-attention call on that sequence alone, and out, lse, dq,
// dk and dv rows are bitwise that call's.  Boundaries are clamped (begin into [0, T], end into
// [begin, T]) so no content of cu makes any address leave the tensors; cu[n] > T truncates the
// last sequence, rows from cu[n] on are never written, anything else unpromised gives unspecified
// values.
//
// P is recomputed in both backward kernels (seven products per tile pair instead of five): no
// atomics, no hand-off between workgroups, every sum has one owner and a fixed order, so all
// five outputs are bitwise reproducible.  Only plain vector stores write global memory.
#include <hip/hip_runtime.h>
#include <pybind11/pybind11.h>

#include <cmath>
#include <stdexcept>
#include <string>
#include <tuple>
#include <type_traits>

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
  // kVarlen reads none of them: there Sq is T and two slots carry the packing instead
  int Sk, q_pos0;
  union { int L; int n; };                 // kSegmented: keys per segment; kVarlen: sequences
  union { int64_t kseg; const int* cu; };  // kSegmented: segment stride of k; kVarlen: boundaries [n + 1]
  int64_t vseg;                            // segment stride of v (kSegmented only)
};

struct BwdArgs {
  const uint16_t *q, *k, *v, *dout;
  const float *lse, *delta;
  uint16_t *dq, *dk, *dv;
  Strides sq, sk, sv, sdo;
  int Sq, Hq, Hkv;
  float scale, scale_log2;
  // the chunk form's own arguments follow those of self-attention, whose layout is unchanged
  // kVarlen reads none of them: there Sq is T and two slots carry the packing instead
  int Sk, q_pos0;
  union { int L; int n; };  // kSegmented: keys per segment; kVarlen: sequences
  Strides sdk, sdv;
  union { int64_t kseg; const int* cu; };  // kSegmented: segment stride of k; kVarlen: boundaries [n + 1]
  int64_t vseg, dkseg, dvseg;              // segment strides of v / dk / dv (kSegmented only)
};

// Instantiations of every kernel.  kSelf is self-attention as it always was: one length (Sk = Sq),
// q_pos0 = 0 and contiguous dk / dv are compile-time facts there, so it keeps its code and its
// speed; kChunk reads Sq, Sk and q_pos0 from the arguments and writes dk / dv through their
// strides; kSegmented adds the segmented key axis; kVarlen is self-attention inside each sequence
// of a packed token axis, the boundaries read from cu.
constexpr int kSelf = 0, kChunk = 1, kSegmented = 2, kVarlen = 3;

// kVarlen: where the workgroup of one slot works.  Sequence i owns rows [begin, begin + len) of the
// token axis, begin = clamp(cu[i], 0, T) and the end clamped into [begin, T], and the slots from
// begin / BLK + i on: the slot's sequence is the last one that starts at or before it (bisection,
// uniform loads), `tile` its BLK-row block inside that sequence.  The slot is spare when the tile
// lies past the sequence (or before it, which only a broken cu produces).
struct Slot {
  int begin, len, tile;
  template <int BLK>
  __device__ __forceinline__ bool spare() const { return tile < 0 || tile * BLK >= len; }
};
template <int BLK>
__device__ __forceinline__ Slot varlen_slot(const int* cu, int n, int T, int slot) {
  auto at = [&](int i) { return min(max(cu[i], 0), T); };
  int lo = 0, hi = n;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (at(mid) / BLK + mid <= slot) lo = mid; else hi = mid;
  }
  const int begin = at(lo), end = max(at(lo + 1), begin);
  return {begin, end - begin, slot - (begin / BLK + lo)};
}

// Element offset of key row `key` on the key axis of k / v / dk / dv.  SEG: the axis is cut into
// segments of L keys, `seg` elements apart (the rank-major layout of an all-gather); otherwise
// one run of stride s.  Applied per key row, so a tile may straddle segments.
template <bool SEG>
__device__ __forceinline__ int64_t key_off(int key, int L, int64_t seg, int64_t s) {
  if (!SEG) return (int64_t)key * s;
  const int n = key / L;
  return (int64_t)n * seg + (int64_t)(key - n * L) * s;
}

// The mask, and everything a kernel concludes from it.  Query row qi sits at position p0 + qi of
// the key sequence; key `key` is visible to it iff both exist and, under CAUSAL, key <= p0 + qi.
// Every skip below is that one rule (`above`) applied to the corner of a block of rows and keys.
template <bool CAUSAL, int MODE>
struct Mask {
  int Sq, Sk, p0;
  template <typename Args>
  __device__ __forceinline__ explicit Mask(const Args& a) : Sq(a.Sq), Sk(MODE ? a.Sk : a.Sq), p0(MODE ? a.q_pos0 : 0) {}
  // kVarlen: self-attention inside one sequence of the packing
  __device__ __forceinline__ explicit Mask(int len) : Sq(len), Sk(len), p0(0) {}
  // key lies above the diagonal of row qi + d
  __device__ __forceinline__ bool above(int qi, int key, int d = 0) const { return CAUSAL && key > p0 + qi + d; }
  // rows past Sq are computed and never stored, so the forward leaves the row test out
  __device__ __forceinline__ bool key_masked(int qi, int key) const { return key >= Sk || above(qi, key); }
  __device__ __forceinline__ bool masked(int qi, int key) const { return qi >= Sq || key >= Sk || above(qi, key); }
  // the `rows` rows from q_first see no key >= key_first: a wave skips the step
  __device__ __forceinline__ bool none_visible(int q_first, int rows, int key_first) const { return above(q_first, key_first, rows - 1); }
  // some row >= q_first does not see some key < key_end: the step needs the per-element test
  __device__ __forceinline__ bool edge(int q_first, int key_end) const { return key_end > Sk || above(q_first, key_end - 1); }
  // forward / dQ: end of the key loop of the kFlashBQ rows from q0 (tiles above the diagonal are skipped)
  __device__ __forceinline__ int key_end(int q0) const { return CAUSAL ? min(Sk, p0 + q0 + kFlashBQ) : Sk; }
  // dK/dV: first kFlashBwdQ-row query step that sees a key >= key0; it may lie past Sq (no steps)
  __device__ __forceinline__ int first_query_step(int key0) const {
    return CAUSAL ? (MODE ? max(0, key0 - p0) : key0) / kFlashBwdQ : 0;
  }
};

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
// Operand fragment kk of query row qi for a product with the query on the MFMA column, from q or
// dout (`p` at the batch and head, row stride `s`; zeros where !ok): the prologue of the forward
// and dQ kernels.
__device__ __forceinline__ bf16x8 ld_query_frag(const uint16_t* p, int64_t s, int qi, int kk, int g, bool ok) {
  return as_frag(ld_g16(p + (int64_t)qi * s + 32 * kk + 8 * g, ok));
}

template <int D, bool CAUSAL, int MODE>
__global__ __launch_bounds__(kFlashThreads) void k_flash_fwd(const FwdArgs a) {
  constexpr int LDK = D + 8, LDT = kFlashBK + 8, KK = D / 32, DT = D / 16;
  constexpr int KP = kFlashBK * (D / 8) / kFlashThreads, VP = D / 32;
  __shared__ __attribute__((aligned(16))) uint16_t Ks[kFlashBK * LDK];
  __shared__ __attribute__((aligned(16))) uint16_t Vt[D * LDT];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = lane & 15, g = lane >> 4;
  const int h = blockIdx.y, b = blockIdx.z;
  constexpr bool SEG = MODE == kSegmented, VAR = MODE == kVarlen;
  Slot sl{0, 0, (int)(gridDim.x - 1 - blockIdx.x)};  // heaviest blocks first
  if constexpr (VAR) {
    sl = varlen_slot<kFlashBQ>(a.cu, a.n, a.Sq, sl.tile);
    if (sl.template spare<kFlashBQ>()) return;
  }
  const int qb = sl.tile;
  const Mask<CAUSAL, MODE> mask = VAR ? Mask<CAUSAL, MODE>(sl.len) : Mask<CAUSAL, MODE>(a);
  const int hk = h / (a.Hq / a.Hkv), Sq = mask.Sq, Sk = mask.Sk;
  const int q0 = qb * kFlashBQ, qw = q0 + wave * (16 * kFlashQT);
  const uint16_t* qp = a.q + b * a.sq.b + h * a.sq.h + sl.begin * a.sq.s;
  const uint16_t* kp = a.k + b * a.sk.b + hk * a.sk.h + sl.begin * a.sk.s;
  const uint16_t* vp = a.v + b * a.sv.b + hk * a.sv.h + sl.begin * a.sv.s;

  bf16x8 qf[kFlashQT][KK];
#pragma unroll
  for (int t = 0; t < kFlashQT; ++t) {
    const int qi = qw + 16 * t + c;
#pragma unroll
    for (int kk = 0; kk < KK; ++kk) qf[t][kk] = ld_query_frag(qp, a.sq.s, qi, kk, g, qi < Sq);
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

  const int nt = (mask.key_end(q0) + kFlashBK - 1) / kFlashBK;
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
    if (mask.none_visible(qw, 16 * kFlashQT, key0)) continue;  // every key above every row of this wave

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
    const bool edge = mask.edge(qw, key0 + kFlashBK);
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
            if (mask.key_masked(qi, key)) x = -INFINITY;
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
    // kVarlen: out [T, Hq, D] and lse [Hq, T] at the sequence's first row
    uint16_t* op = a.out + (((VAR ? (int64_t)sl.begin : (int64_t)b * Sq) + qi) * a.Hq + h) * D + 4 * g;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) st_g8(op + 16 * dt, o[t][dt], inv);
    if (g == 0)
      a.lse[(VAR ? (int64_t)h * a.Sq + sl.begin : ((int64_t)b * a.Hq + h) * Sq) + qi] = (m[t] + __log2f(lt)) * kLn2;
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
  const int hk = blockIdx.y, b = blockIdx.z;
  constexpr bool SEG = MODE == kSegmented, VAR = MODE == kVarlen;
  Slot sl{0, 0, (int)blockIdx.x};
  if constexpr (VAR) {
    sl = varlen_slot<kFlashBK>(a.cu, a.n, a.Sq, sl.tile);
    if (sl.template spare<kFlashBK>()) return;
  }
  const int kb = sl.tile;
  const Mask<CAUSAL, MODE> mask = VAR ? Mask<CAUSAL, MODE>(sl.len) : Mask<CAUSAL, MODE>(a);
  const int Sq = mask.Sq, Sk = mask.Sk, rep = a.Hq / a.Hkv;
  const int key0 = kb * kFlashBK, kw = key0 + 16 * wave, keyi = kw + c;
  const uint16_t* kp = a.k + b * a.sk.b + hk * a.sk.h + sl.begin * a.sk.s + key_off<SEG>(keyi, a.L, a.kseg, a.sk.s);
  const uint16_t* vp = a.v + b * a.sv.b + hk * a.sv.h + sl.begin * a.sv.s + key_off<SEG>(keyi, a.L, a.vseg, a.sv.s);
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
  const int qs0 = mask.first_query_step(key0);
  const int nqs = (Sq + kFlashBwdQ - 1) / kFlashBwdQ - qs0, nq = MODE ? max(0, nqs) : nqs;
  const int steps = rep * nq;  // query heads in order, query steps in order inside each
  const int row = tid & 31, cb = tid >> 5;
  uint4 qr[NP], dr[NP];
  float lv = 0.f, dl = 0.f;
  auto fetch = [&](int i) {
    const int h = hk * rep + i / nq, qi = (qs0 + i % nq) * kFlashBwdQ + row;
    const bool ok = qi < Sq;
    const uint16_t* qp = a.q + b * a.sq.b + h * a.sq.h + ((int64_t)sl.begin + qi) * a.sq.s;
    const uint16_t* dp = a.dout + b * a.sdo.b + h * a.sdo.h + ((int64_t)sl.begin + qi) * a.sdo.s;
#pragma unroll
    for (int j = 0; j < NP; ++j) {
      qr[j] = ld_g16(qp + (cb + 8 * j) * 8, ok);
      dr[j] = ld_g16(dp + (cb + 8 * j) * 8, ok);
    }
    if (tid < kFlashBwdQ) {
      const int64_t o = (VAR ? (int64_t)h * a.Sq + sl.begin : ((int64_t)b * a.Hq + h) * Sq) + qi;
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
    if (mask.none_visible(qbase, kFlashBwdQ, kw)) continue;  // every query of the step before every key of this wave

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
        const float pv = mask.masked(qi, keyi) ? 0.f : fast_exp2(sa[r] * a.scale_log2 - l4[r]);
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
    // self-attention: dk / dv are contiguous [B, S, Hkv, D]; kVarlen: contiguous [T, Hkv, D]
    constexpr bool DENSE = MODE == kSelf || VAR;
    const int64_t o = DENSE ? (((VAR ? (int64_t)sl.begin : (int64_t)b * Sk) + keyi) * a.Hkv + hk) * D : 0;
    uint16_t* dkp = a.dk + (DENSE ? o : b * a.sdk.b + hk * a.sdk.h + key_off<SEG>(keyi, a.L, a.dkseg, a.sdk.s)) + 4 * g;
    uint16_t* dvp = a.dv + (DENSE ? o : b * a.sdv.b + hk * a.sdv.h + key_off<SEG>(keyi, a.L, a.dvseg, a.sdv.s)) + 4 * g;
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
  const int h = blockIdx.y, b = blockIdx.z;
  constexpr bool SEG = MODE == kSegmented, VAR = MODE == kVarlen;
  Slot sl{0, 0, (int)(gridDim.x - 1 - blockIdx.x)};
  if constexpr (VAR) {
    sl = varlen_slot<kFlashBQ>(a.cu, a.n, a.Sq, sl.tile);
    if (sl.template spare<kFlashBQ>()) return;
  }
  const int qb = sl.tile;
  const Mask<CAUSAL, MODE> mask = VAR ? Mask<CAUSAL, MODE>(sl.len) : Mask<CAUSAL, MODE>(a);
  const int hk = h / (a.Hq / a.Hkv), Sq = mask.Sq, Sk = mask.Sk;
  const int q0 = qb * kFlashBQ, qw = q0 + wave * (16 * kFlashQT);
  const uint16_t* qp = a.q + b * a.sq.b + h * a.sq.h + sl.begin * a.sq.s;
  const uint16_t* dop = a.dout + b * a.sdo.b + h * a.sdo.h + sl.begin * a.sdo.s;
  const uint16_t* kp = a.k + b * a.sk.b + hk * a.sk.h + sl.begin * a.sk.s;
  const uint16_t* vp = a.v + b * a.sv.b + hk * a.sv.h + sl.begin * a.sv.s;

  bf16x8 qf[kFlashQT][KK], dof[kFlashQT][KK];
  float lse2[kFlashQT], dl[kFlashQT];
  f4 dq[kFlashQT][DT];
#pragma unroll
  for (int t = 0; t < kFlashQT; ++t) {
    const int qi = qw + 16 * t + c;
    const bool ok = qi < Sq;
#pragma unroll
    for (int kk = 0; kk < KK; ++kk) {
      qf[t][kk] = ld_query_frag(qp, a.sq.s, qi, kk, g, ok);
      dof[t][kk] = ld_query_frag(dop, a.sdo.s, qi, kk, g, ok);
    }
    const int64_t o = (VAR ? (int64_t)h * a.Sq + sl.begin : ((int64_t)b * a.Hq + h) * Sq) + qi;
    lse2[t] = ok ? a.lse[o] * kLog2e : 0.f;
    dl[t] = ok ? a.delta[o] : 0.f;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) dq[t][dt] = f4{0.f, 0.f, 0.f, 0.f};
  }

  const int nt = (mask.key_end(q0) + kFlashBK - 1) / kFlashBK;
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
    if (mask.none_visible(qw, 16 * kFlashQT, key0)) continue;

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
            const float pv = mask.masked(qi, key) ? 0.f : fast_exp2(sa[r] * a.scale_log2 - lse2[t]);
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
    uint16_t* op = a.dq + (((VAR ? (int64_t)sl.begin : (int64_t)b * Sq) + qi) * a.Hq + h) * D + 4 * g;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) st_g8(op + 16 * dt, dq[t][dt], a.scale);
  }
}

// One strided operand as the binding takes it: (address, segment stride, batch, row and head stride),
// strides in elements; the segment stride is 0 where the key axis is one run.
using View = std::tuple<uint64_t, int64_t, int64_t, int64_t, int64_t>;

struct Problem {
  int B;
  int64_t Sq, Sk, L, q_pos0;  // L: keys per segment, = Sk for one run
  int Hq, Hkv, D;
  bool causal;
  double scale;
  bool self;  // the caller's flag: run kSelf
  // the packed form (run kVarlen): the device address of the n + 1 boundaries, else 0; the token
  // axis is Sq = Sk = L = T of B = 1
  uint64_t cu = 0;
  int64_t n = 0;
};

constexpr int64_t kFlashMaxSeqs = 65536;

[[noreturn]] void refuse(const std::string& what) { throw std::invalid_argument("flash_attention: " + what); }

void check(const Problem& p) {
  if (p.D != 64 && p.D != 128) refuse("head dim must be 64 or 128");
  if (p.B < 1 || p.B > 65535 || p.Hq < 1 || p.Hq > 65535) refuse("1 <= B, Hq <= 65535 required");
  if (p.Hkv < 1 || p.Hq % p.Hkv) refuse("Hq must be a multiple of Hkv");
  if (p.Sq < 1 || p.Sq > (1 << 30) || p.Sk < 1 || p.Sk > (1 << 30)) refuse("1 <= Sq, Sk <= 2^30 required");
  if (p.q_pos0 < 0 || p.q_pos0 + p.Sq > (1 << 30)) refuse("0 <= q_pos0 and q_pos0 + Sq <= 2^30 required");
  if (p.L < 1 || p.Sk % p.L) refuse("Sk must be a multiple of the segment length");
  // kSelf takes Sk = Sq and q_pos0 = 0 as compile-time facts and reads neither from the arguments
  if (p.self && (p.Sq != p.Sk || p.L != p.Sk || p.q_pos0 != 0))
    refuse("self-attention needs Sq = Sk = seg_len and q_pos0 = 0");
  if (!p.cu && p.n) refuse("sequences without cu_seqlens");
  if (p.cu) {
    // kVarlen takes one token axis of T rows and reads n + 1 boundaries; T / BLK + n slots fit any grid
    if (p.cu % 4) refuse("cu_seqlens must be 4-byte aligned");
    if (p.n < 1 || p.n > kFlashMaxSeqs) refuse("1 <= n <= 65536 sequences required");
    if (p.self || p.B != 1 || p.Sq != p.Sk || p.L != p.Sk || p.q_pos0 != 0)
      refuse("the packed form needs B = 1, Sq = Sk = seg_len = T, q_pos0 = 0 and no self_attention flag");
  }
}

// Checks a view and unpacks it into the kernel arguments.
template <typename T>
void take(const char* what, const View& v, T*& ptr, Strides& st, int64_t* seg = nullptr) {
  const auto [p, sg, b, s, h] = v;
  if (p == 0 || p % 16) refuse(std::string(what) + " must be 16-byte aligned");
  if (b % 8 || s % 8 || h % 8) refuse(std::string(what) + " strides must be multiples of 8 elements");
  if (sg % 8) refuse(std::string("segment stride of ") + what + " must be a multiple of 8 elements");
  ptr = reinterpret_cast<T*>(p);
  st = {b, s, h};
  if (seg) *seg = sg;
}

// The fields FwdArgs and BwdArgs share.
template <typename Args>
void fill(Args& a, const Problem& p, const View& q, const View& k, const View& v) {
  check(p);
  take("q", q, a.q, a.sq);
  take("k", k, a.k, a.sk, &a.kseg);
  take("v", v, a.v, a.sv, &a.vseg);
  a.Sq = (int)p.Sq;
  a.Sk = (int)p.Sk;
  a.L = (int)p.L;
  if (p.cu) {  // the two slots kVarlen reads instead (Sq is T)
    a.n = (int)p.n;
    a.cu = reinterpret_cast<const int*>(p.cu);
  }
  a.q_pos0 = (int)p.q_pos0;
  a.Hq = p.Hq;
  a.Hkv = p.Hkv;
  a.scale_log2 = (float)(p.scale * 1.4426950408889634);
}

// Calls f(D, causal, MODE) with the kernels' compile-time values as integral constants.  The mode
// is the caller's: kSelf on its flag, kVarlen with boundaries, else kChunk, or kSegmented when the
// key axis is segmented.
template <typename F>
void dispatch(const Problem& p, F&& f) {
  auto by_mode = [&](auto d, auto c) {
    if (p.self) f(d, c, std::integral_constant<int, kSelf>{});
    else if (p.cu) f(d, c, std::integral_constant<int, kVarlen>{});
    else if (p.L == p.Sk) f(d, c, std::integral_constant<int, kChunk>{});
    else f(d, c, std::integral_constant<int, kSegmented>{});
  };
  auto by_causal = [&](auto d) {
    if (p.causal) by_mode(d, std::true_type{}); else by_mode(d, std::false_type{});
  };
  if (p.D == 64) by_causal(std::integral_constant<int, 64>{}); else by_causal(std::integral_constant<int, 128>{});
}

// Workgroups along a `rows`-long axis cut into blocks of `blk`; the packed form has T / blk + n slots
// whatever the boundaries hold.
unsigned blocks(const Problem& p, int64_t rows, int blk) {
  return (unsigned)(p.cu ? rows / blk + p.n : (rows + blk - 1) / blk);
}
dim3 query_grid(const Problem& p) { return dim3(blocks(p, p.Sq, kFlashBQ), (unsigned)p.Hq, (unsigned)p.B); }

void flash_attn_fwd(const View& q, const View& k, const View& v, uint64_t out, uint64_t lse, int B, int64_t Sq, int64_t Sk,
                    int64_t seg_len, int64_t q_pos0, int Hq, int Hkv, int D, bool causal, double scale, bool self_attention,
                    uint64_t stream, uint64_t cu_seqlens, int64_t n_seq) {
  const Problem p{B, Sq, Sk, seg_len, q_pos0, Hq, Hkv, D, causal, scale, self_attention, cu_seqlens, n_seq};
  FwdArgs a;
  fill(a, p, q, k, v);
  if (out == 0 || out % 16 || lse == 0 || lse % 4) refuse("misaligned out / lse");
  a.out = reinterpret_cast<uint16_t*>(out);
  a.lse = reinterpret_cast<float*>(lse);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  dispatch(p, [&](auto d, auto c, auto m) {
    hipLaunchKernelGGL((k_flash_fwd<decltype(d)::value, decltype(c)::value, decltype(m)::value>), query_grid(p),
                       dim3(kFlashThreads), 0, st, a);
  });
  CCMPI_HIP_CHECK(hipGetLastError());
}

void flash_attn_bwd(const View& dout, const View& q, const View& k, const View& v, uint64_t out, uint64_t lse,
                    uint64_t delta, uint64_t dq, const View& dk, const View& dv, int B, int64_t Sq, int64_t Sk,
                    int64_t seg_len, int64_t q_pos0, int Hq, int Hkv, int D, bool causal, double scale, bool self_attention,
                    uint64_t stream, uint64_t cu_seqlens, int64_t n_seq) {
  const Problem p{B, Sq, Sk, seg_len, q_pos0, Hq, Hkv, D, causal, scale, self_attention, cu_seqlens, n_seq};
  BwdArgs a;
  fill(a, p, q, k, v);
  if (Hkv > 65535) refuse("Hkv <= 65535 required");  // a grid dimension of the dK/dV kernel
  take("dout", dout, a.dout, a.sdo);
  take("dk", dk, a.dk, a.sdk, &a.dkseg);
  take("dv", dv, a.dv, a.sdv, &a.dvseg);
  if (self_attention || cu_seqlens) {
    // the kSelf and kVarlen dK/dV stores ignore the strides: they must be those of a contiguous
    // [B, S, Hkv, D] tensor (0 stands for the stride of an axis of length 1)
    const Strides want{Sk * Hkv * D, (int64_t)Hkv * D, (int64_t)D};
    auto same = [](int64_t got, int64_t w, int64_t len) { return got == w || (len == 1 && got == 0); };
    for (const Strides* s : {&a.sdk, &a.sdv})
      if (!same(s->b, want.b, B) || !same(s->s, want.s, Sk) || !same(s->h, want.h, Hkv))
        refuse("self-attention and the packed form need contiguous dk / dv");
  }
  if (out == 0 || (out | dq) % 16 || dq == 0 || lse == 0 || delta == 0 || (lse | delta) % 4)
    refuse("misaligned out / lse / delta / dq");
  const int64_t rows = (int64_t)B * Sq * Hq;
  const int64_t dblocks = (rows + 16 * (kFlashThreads / 64) - 1) / (16 * (kFlashThreads / 64));
  if (dblocks > 0x7fffffffLL) refuse("B * S * Hq too large");
  const uint16_t* outp = reinterpret_cast<const uint16_t*>(out);
  float* deltap = reinterpret_cast<float*>(delta);
  a.lse = reinterpret_cast<const float*>(lse);
  a.delta = deltap;
  a.dq = reinterpret_cast<uint16_t*>(dq);
  a.scale = (float)scale;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const dim3 block(kFlashThreads), key_grid(blocks(p, Sk, kFlashBK), (unsigned)Hkv, (unsigned)B);
  dispatch(p, [&](auto d, auto c, auto m) {
    constexpr int DD = decltype(d)::value, M = decltype(m)::value;
    constexpr bool C = decltype(c)::value;
    hipLaunchKernelGGL(k_flash_delta<DD>, dim3((unsigned)dblocks), block, 0, st, a.dout, a.sdo, outp, deltap, rows, a.Sq, a.Hq);
    hipLaunchKernelGGL((k_flash_bwd_dkv<DD, C, M>), key_grid, block, 0, st, a);
    hipLaunchKernelGGL((k_flash_bwd_dq<DD, C, M>), query_grid(p), block, 0, st, a);
  });
  CCMPI_HIP_CHECK(hipGetLastError());
}

}  // namespace

void register_flash_attn_ops(pybind11::module_& m) {
  namespace py = pybind11;
  m.attr("FLASH_BQ") = kFlashBQ;
  m.attr("FLASH_BK") = kFlashBK;
  m.def("flash_attn_fwd", &flash_attn_fwd,
        "forward: q [B, Sq, Hq, D] at positions q_pos0.., k / v with Sk keys in segments of seg_len; each a bf16 view "
        "(address, segment stride, b, s, h strides in elements; unit stride on D).  causal: key j visible to row i iff "
        "j <= q_pos0 + i -> out [B, Sq, Hq, D] bf16 contiguous, lse [B, Hq, Sq] fp32.  self_attention: the "
        "self-attention kernels (Sq = Sk = seg_len, q_pos0 = 0).  cu_seqlens (device address of n_seq + 1 int32 "
        "boundaries): the packed form, B = 1 and Sq = Sk = seg_len = T tokens, self-attention inside each sequence; "
        "out [T, Hq, D], lse [Hq, T]",
        py::arg("q"), py::arg("k"), py::arg("v"), py::arg("out"), py::arg("lse"), py::arg("B"), py::arg("Sq"),
        py::arg("Sk"), py::arg("seg_len"), py::arg("q_pos0"), py::arg("Hq"), py::arg("Hkv"), py::arg("D"),
        py::arg("causal"), py::arg("scale"), py::arg("self_attention"), py::arg("stream"), py::arg("cu_seqlens") = 0,
        py::arg("n_seq") = 0, py::call_guard<py::gil_scoped_release>());
  m.def("flash_attn_bwd", &flash_attn_bwd,
        "backward: delta [B, Hq, Sq] fp32 workspace, dq [B, Sq, Hq, D] bf16 contiguous; dk / dv views like k / v, "
        "written through their own strides (a key no query sees gets exact zeros), contiguous [B, S, Hkv, D] with "
        "self_attention and in the packed form (cu_seqlens, n_seq as in the forward: delta [Hq, T], dq [T, Hq, D], "
        "dk / dv [T, Hkv, D]); three launches (delta, dK/dV, dQ), no atomics",
        py::arg("dout"), py::arg("q"), py::arg("k"), py::arg("v"), py::arg("out"), py::arg("lse"), py::arg("delta"),
        py::arg("dq"), py::arg("dk"), py::arg("dv"), py::arg("B"), py::arg("Sq"), py::arg("Sk"), py::arg("seg_len"),
        py::arg("q_pos0"), py::arg("Hq"), py::arg("Hkv"), py::arg("D"), py::arg("causal"), py::arg("scale"),
        py::arg("self_attention"), py::arg("stream"), py::arg("cu_seqlens") = 0, py::arg("n_seq") = 0,
        py::call_guard<py::gil_scoped_release>());
}

}  // namespace dev
}  // namespace ccmpi
