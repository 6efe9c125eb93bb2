// Routed MoE token dispatch and weighted combine over IPC-mapped peer HBM.
//
// p ranks, E experts, El = E / p consecutive experts per rank.  Every rank holds
// x [T, D] and the router's topk_idx [T, K] (-1 = slot dropped); the flat entry
// index of (token t, slot k) is f = t * K + k.
//
//   routing  (local)       k_moe_hist + k_moe_rank: this rank's per-expert counts
//                          C_me[E], staged at the start of its scratch segment, and
//                          for every entry its stable rank among this rank's entries
//                          of the same expert (order of f).  Counts come from LDS
//                          atomics; positions never depend on their order: chunks of
//                          kMoeChunk entries, a prefix over the chunk histograms per
//                          expert, and inside a chunk thread e numbers the entries
//                          equal to e while it walks the chunk (broadcast LDS reads).
//   dispatch (collective)  k_moe_dispatch: after the start barrier every CTA reads all
//                          p count rows (and capacities) into LDS, derives
//                            base(e) = sum_{e' < e on e's rank} sum_i C[i][e'] + sum_{i < me} C[i][e]
//                          and pushes x[t] into the owner's recv_x at row base + pos for
//                          each routed slot: the row is loaded once and stored up to K
//                          times (posted 16-B system-coherent writes).  Rows end up in
//                          (local expert, source rank, token, slot) order whatever the
//                          scheduling.  A row past the owner's capacity is not written
//                          (fault code 0xA00 + owner, row_of = -1).
//                          With an expert capacity Ce (MoEArgs::expert_cap, rank-invariant)
//                          expert e keeps its first Ce entries in that order: entry pos of
//                          this rank is kept iff before(e) + pos < Ce, the expert has
//                          col'(e) = min(col(e), Ce) rows and base uses col'.  All of it is
//                          closed-form from the count matrix in LDS: no exchange, no atomics.
//                          A dropped entry gets row_of = -1, is not written and records no
//                          fault; CTA 0 writes this rank's number of them to num_dropped.
//   combine  (collective)  k_moe_combine: the start barrier publishes y; one wave per
//                          token issues the loads of its K rows (peer memory) before
//                          the fp32 multiply-add chain in slot order, rounds once and
//                          stores out[t].  No atomics, no [T * K, D] staging.
//   combine backward       k_moe_combine_bwd: the start barrier publishes y (read from
//   (collective)           peers) and dy (written into peers); one wave per token loads
//                          dout[t] once, pushes w[t,k] * dout[t] (one fp32 multiply, one
//                          rounding; a plain copy without weights) into the owner's dy at
//                          row_of[t,k], and, when dweights is wanted, pulls the K rows of y
//                          for dweights[t,k] = <dout[t], y row>: fp32 per lane in vector
//                          order, then a fixed butterfly over the wave (reproducible).
//                          Rows are a bijection, so every routed row of dy is written once;
//                          rows past a rank's total stay untouched.  An owner that published
//                          no y while this rank pulls: its dy rows are read instead (in
//                          bounds) and the call fails (fault code 0xD00 + owner).
//
// The grid is the same on every rank (CTA b pairs with CTA b of the peers); T may
// differ per rank and be 0, such a rank still runs the barriers.
#include "common.hpp"
#include "moe.hpp"
#include "phase.hpp"

namespace ccmpi {
namespace dev {

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
static_assert(kThreads == kMoeMaxExperts, "one thread per expert");
static_assert(kMoeChunk % kThreads == 0 && kMoeChunk % 4 == 0, "chunk layout");

__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }

// ---------------------------------------------------------------------------
// routing
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(kThreads) k_moe_hist(MoEArgs m) {
  __shared__ int32_t h[kMoeMaxExperts];
  const int t = threadIdx.x;
  const int64_t n = (int64_t)m.T * m.K;
  h[t] = 0;
  __syncthreads();
  const int64_t f0 = (int64_t)blockIdx.x * kMoeChunk;
  for (int i = t; i < kMoeChunk; i += kThreads) {
    if (f0 + i < n) {
      const int e = m.idx[f0 + i];
      if (e >= 0 && e < m.E) atomicAdd(&h[e], 1);
    }
  }
  __syncthreads();
  if (t < m.E) m.chunk_hist[(int64_t)blockIdx.x * m.E + t] = h[t];
}

// CTA c numbers the entries of chunk c; CTA 0 also writes the count row.
__global__ void __launch_bounds__(kThreads) k_moe_rank(MoEArgs m, int nchunks) {
  __shared__ __attribute__((aligned(16))) int32_t s_idx[kMoeChunk];
  __shared__ int32_t s_pos[kMoeChunk];
  const int t = threadIdx.x, c = blockIdx.x;
  const int64_t n = (int64_t)m.T * m.K;
  const int64_t f0 = (int64_t)c * kMoeChunk;
  for (int i = t; i < kMoeChunk; i += kThreads) {
    int e = -1;
    if (f0 + i < n) {
      e = m.idx[f0 + i];
      if (e < 0 || e >= m.E) e = -1;
    }
    s_idx[i] = e;
  }
  int run = 0;
  if (t < m.E) {
    for (int cc = 0; cc < c; ++cc) run += m.chunk_hist[(int64_t)cc * m.E + t];
    if (c == 0) {
      int total = 0;
      for (int cc = 0; cc < nchunks; ++cc) total += m.chunk_hist[(int64_t)cc * m.E + t];
      m.count_row[t] = total;
    }
  }
  __syncthreads();
  if (t < m.E) {
    typedef int i32x4 __attribute__((ext_vector_type(4)));
    for (int q = 0; q < kMoeChunk / 4; ++q) {
      const i32x4 v = reinterpret_cast<const i32x4*>(s_idx)[q];  // same address in every lane: broadcast
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (v[u] == t) s_pos[q * 4 + u] = run++;
    }
  }
  __syncthreads();
  for (int i = t; i < kMoeChunk; i += kThreads)
    if (f0 + i < n) m.row_of[f0 + i] = s_idx[i] >= 0 ? s_pos[i] : -1;
}

// ---------------------------------------------------------------------------
// dispatch
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(kThreads) k_moe_dispatch(MoEArgs m) {
  __shared__ uint64_t s_epoch;
  __shared__ uint64_t codes[2][kMaxRanks];
  __shared__ int32_t C[kMaxRanks * kMoeMaxExperts];  // C[i * E + e]: rank i's entries for expert e
  __shared__ int32_t s_col[kMoeMaxExperts], s_before[kMoeMaxExperts], s_base[kMoeMaxExperts];
  __shared__ int32_t s_cap[kMaxRanks];
  __shared__ int32_t s_drop[kMoeMaxExperts];  // this rank's entries of expert e over the expert capacity
  __shared__ char* s_out[kMaxRanks];
  const CollArgs& a = m.a;
  const PeerTable* pt = a.pt;
  const int E = m.E, El = m.El, K = m.K;
  const int Ce = m.expert_cap;  // rows kept per expert, 0 = no limit
  if (threadIdx.x == 0) {  // published with the start barrier (thread 0 releases before its flag)
    int32_t* mine = reinterpret_cast<int32_t*>(resolve(pt, pt->rank, a.src_code));
    __hip_atomic_store(mine + E, m.cap, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
  if (!start_phase(a, &s_epoch, codes)) return;
  const uint64_t e0 = s_epoch;
  const int me = pt->rank, nr = pt->size;
  for (int t = threadIdx.x; t < nr * (E + 1); t += kThreads) {
    const int i = t / (E + 1), j = t % (E + 1);
    const int32_t* row = reinterpret_cast<const int32_t*>(resolve(pt, i, codes[0][i]));
    const int32_t v = __hip_atomic_load(row + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    if (j < E) C[i * E + j] = v;
    else s_cap[i] = v;
  }
  if (threadIdx.x < nr) s_out[threadIdx.x] = resolve(pt, threadIdx.x, codes[1][threadIdx.x]);
  __syncthreads();
  if (threadIdx.x < E) {
    int col = 0, before = 0;
    for (int i = 0; i < nr; ++i) {
      const int v = C[i * E + threadIdx.x];
      col += v;
      if (i < me) before += v;
    }
    if (Ce > 0) {
      // an expert keeps its first Ce entries in (source rank, token, slot) order: this rank's
      // entry pos is kept iff before + pos < Ce, so it keeps clamp(Ce - before, 0, C[me][e])
      const int mine = C[me * E + threadIdx.x];
      s_drop[threadIdx.x] = mine - min(max(Ce - before, 0), mine);
      col = min(col, Ce);
    }
    s_col[threadIdx.x] = col;
    s_before[threadIdx.x] = before;  // not clamped: only read for kept entries, where before < Ce
  }
  __syncthreads();
  if (threadIdx.x < E) {
    int b = s_before[threadIdx.x];
    for (int ee = threadIdx.x / El * El; ee < (int)threadIdx.x; ++ee) b += s_col[ee];
    s_base[threadIdx.x] = b;
  }
  if (blockIdx.x == 0 && threadIdx.x < El) m.expert_counts[threadIdx.x] = s_col[me * El + threadIdx.x];
  if (blockIdx.x == 0 && threadIdx.x < 64 && m.num_dropped) {  // wave 0: a fixed butterfly, no atomics
    int d = 0;
    if (Ce > 0)
      for (int ee = threadIdx.x; ee < E; ee += 64) d += s_drop[ee];
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) d += __shfl_xor(d, s, 64);
    if (threadIdx.x == 0) *m.num_dropped = d;
  }
  __syncthreads();

  const int lane = threadIdx.x & 63;
  const int gw = blockIdx.x * kWaves + (threadIdx.x >> 6), nw = gridDim.x * kWaves;
  const uint32_t nv = m.row_bytes / 16;
  for (int t = gw; t < m.T; t += nw) {
    Rsrc dst[kMoeMaxTopK];
    bool on[kMoeMaxTopK];
#pragma unroll
    for (int k = 0; k < kMoeMaxTopK; ++k) {
      on[k] = false;
      if (k < K) {
        const int64_t f = (int64_t)t * K + k;
        const int pos = uni(m.row_of[f]);
        if (pos >= 0) {
          const int e = uni(m.idx[f]);
          const int owner = e / El;
          const int row = uni(s_base[e]) + pos;
          const bool kept = Ce <= 0 || uni(s_before[e]) + pos < Ce;  // over the expert capacity: dropped, no fault
          on[k] = kept && row < uni(s_cap[owner]);
          if (on[k]) {
            dst[k] = make_rsrc(uniform_ptr(s_out[owner] + (uint64_t)row * m.row_bytes), m.row_bytes);
          } else if (kept && lane == 0) {
            __hip_atomic_store(&pt->sig[me]->error, 0xA00u + owner, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            report_host(pt, 0xA00u + owner);
          }
          if (lane == 0) m.row_of[f] = on[k] ? row : -1;
        }
      }
    }
    const u32x4* src = reinterpret_cast<const u32x4*>(a.in + (uint64_t)t * m.row_bytes);
    for (uint32_t v0 = lane; v0 < nv; v0 += 64 * 4) {
      u32x4 x[4];
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (v0 + u * 64 < nv) x[u] = src[v0 + u * 64];
#pragma unroll
      for (int k = 0; k < kMoeMaxTopK; ++k) {
        if (on[k]) {
#pragma unroll
          for (int u = 0; u < 4; ++u)
            if (v0 + u * 64 < nv) st16(dst[k], (v0 + u * 64) * 16, x[u]);
        }
      }
    }
  }
  if (!sync_phase(a, 3, e0)) return;
  finish(a, e0);
}

// ---------------------------------------------------------------------------
// combine
// ---------------------------------------------------------------------------
template <int DT> struct Row16;
template <> struct Row16<DT_F32> {
  static constexpr int N = 4;
  __device__ static void unpack(u32x4 x, float* f) { for (int i = 0; i < 4; ++i) f[i] = __uint_as_float(x[i]); }
  __device__ static u32x4 pack(const float* f) { u32x4 r; for (int i = 0; i < 4; ++i) r[i] = __float_as_uint(f[i]); return r; }
};
template <> struct Row16<DT_BF16> {
  static constexpr int N = 8;
  __device__ static void unpack(u32x4 x, float* f) {
    for (int i = 0; i < 4; ++i) { f[2 * i] = bf16_lo(x[i]); f[2 * i + 1] = bf16_hi(x[i]); }
  }
  __device__ static u32x4 pack(const float* f) { u32x4 r; for (int i = 0; i < 4; ++i) r[i] = pk_bf16(f[2 * i], f[2 * i + 1]); return r; }
};
template <> struct Row16<DT_F16> {
  static constexpr int N = 8;
  using V = VecAcc<DT_F16>;
  __device__ static void unpack(u32x4 x, float* f) {
    for (int i = 0; i < 4; ++i) { f[2 * i] = V::h2f(x[i] & 0xffff); f[2 * i + 1] = V::h2f(x[i] >> 16); }
  }
  __device__ static u32x4 pack(const float* f) {
    u32x4 r; for (int i = 0; i < 4; ++i) r[i] = V::f2h(f[2 * i]) | (V::f2h(f[2 * i + 1]) << 16); return r;
  }
};

template <int DT>
__global__ void __launch_bounds__(kThreads) k_moe_combine(MoEArgs m) {
  __shared__ uint64_t s_epoch;
  __shared__ uint64_t codes[2][kMaxRanks];
  __shared__ char* s_y[kMaxRanks];
  const CollArgs& a = m.a;
  const PeerTable* pt = a.pt;
  if (!start_phase(a, &s_epoch, codes)) return;
  const uint64_t e0 = s_epoch;
  const int nr = pt->size, E = m.E, El = m.El, K = m.K;
  if (threadIdx.x < nr) s_y[threadIdx.x] = resolve(pt, threadIdx.x, codes[0][threadIdx.x]);
  __syncthreads();

  using R = Row16<DT>;
  constexpr int U = 2;
  const int lane = threadIdx.x & 63;
  const int gw = blockIdx.x * kWaves + (threadIdx.x >> 6), nw = gridDim.x * kWaves;
  const uint32_t nv = m.row_bytes / 16;
  for (int t = gw; t < m.T; t += nw) {
    Rsrc src[kMoeMaxTopK];
    bool on[kMoeMaxTopK];
    float w[kMoeMaxTopK];
#pragma unroll
    for (int k = 0; k < kMoeMaxTopK; ++k) {
      on[k] = false;
      w[k] = 1.0f;
      if (k < K) {
        const int64_t f = (int64_t)t * K + k;
        const int row = uni(m.row_of[f]);
        const int e = uni(m.idx[f]);
        on[k] = row >= 0 && e >= 0 && e < E;
        if (on[k]) {
          src[k] = make_rsrc(uniform_ptr(s_y[e / El] + (uint64_t)row * m.row_bytes), m.row_bytes);
          if (m.weights) w[k] = __uint_as_float((uint32_t)uni((int)__float_as_uint(m.weights[f])));
        }
      }
    }
    u32x4* out = reinterpret_cast<u32x4*>(a.out + (uint64_t)t * m.row_bytes);
    for (uint32_t v0 = lane; v0 < nv; v0 += 64 * U) {
      u32x4 y[U][kMoeMaxTopK];
      // every slot's (peer) load in flight before the first use
#pragma unroll
      for (int k = 0; k < kMoeMaxTopK; ++k) {
        if (on[k]) {
#pragma unroll
          for (int u = 0; u < U; ++u)
            if (v0 + u * 64 < nv) y[u][k] = ld16(src[k], (v0 + u * 64) * 16);
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (v0 + u * 64 < nv) {
          float acc[R::N];
#pragma unroll
          for (int i = 0; i < R::N; ++i) acc[i] = 0.0f;
#pragma unroll
          for (int k = 0; k < kMoeMaxTopK; ++k) {  // slot order, fp32
            if (on[k]) {
              float v[R::N];
              R::unpack(y[u][k], v);
#pragma unroll
              for (int i = 0; i < R::N; ++i) acc[i] = __builtin_fmaf(w[k], v[i], acc[i]);
            }
          }
          out[v0 + u * 64] = R::pack(acc);
        }
      }
    }
  }
  if (!sync_phase(a, 3, e0)) return;
  finish(a, e0);
}

// ---------------------------------------------------------------------------
// combine backward
// ---------------------------------------------------------------------------
// Sum over the 64 lanes in a fixed butterfly: every lane ends with the same bits,
// whatever the scheduling.
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor(v, s, 64);
  return v;
}

template <int DT, bool PULL>
__global__ void __launch_bounds__(kThreads) k_moe_combine_bwd(MoEArgs m) {
  __shared__ uint64_t s_epoch;
  __shared__ uint64_t codes[2][kMaxRanks];
  __shared__ char* s_y[kMaxRanks];
  __shared__ char* s_dy[kMaxRanks];
  const CollArgs& a = m.a;
  const PeerTable* pt = a.pt;
  if (!start_phase(a, &s_epoch, codes)) return;
  const uint64_t e0 = s_epoch;
  const int nr = pt->size, E = m.E, El = m.El, K = m.K;
  if (threadIdx.x < nr) {
    s_dy[threadIdx.x] = resolve(pt, threadIdx.x, codes[1][threadIdx.x]);
    s_y[threadIdx.x] = nullptr;
    if (PULL) {
      if (codes[0][threadIdx.x]) {
        s_y[threadIdx.x] = resolve(pt, threadIdx.x, codes[0][threadIdx.x]);
      } else {  // that rank was given no y (code 0): its dy rows are read instead, in bounds, and the call fails
        s_y[threadIdx.x] = s_dy[threadIdx.x];
        __hip_atomic_store(&pt->sig[pt->rank]->error, 0xD00u + threadIdx.x, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_SYSTEM);
        report_host(pt, 0xD00u + threadIdx.x);
      }
    }
  }
  __syncthreads();

  using R = Row16<DT>;
  constexpr int U = 2;
  const int lane = threadIdx.x & 63;
  const int gw = blockIdx.x * kWaves + (threadIdx.x >> 6), nw = gridDim.x * kWaves;
  const uint32_t nv = m.row_bytes / 16;
  const bool scaled = m.weights != nullptr;
  for (int t = gw; t < m.T; t += nw) {
    Rsrc src[kMoeMaxTopK], dst[kMoeMaxTopK];
    bool on[kMoeMaxTopK];
    float w[kMoeMaxTopK], dot[kMoeMaxTopK];
#pragma unroll
    for (int k = 0; k < kMoeMaxTopK; ++k) {
      on[k] = false;
      w[k] = 1.0f;
      dot[k] = 0.0f;
      if (k < K) {
        const int64_t f = (int64_t)t * K + k;
        const int row = uni(m.row_of[f]);
        const int e = uni(m.idx[f]);
        on[k] = row >= 0 && e >= 0 && e < E;
        if (on[k]) {
          const uint64_t off = (uint64_t)row * m.row_bytes;
          dst[k] = make_rsrc(uniform_ptr(s_dy[e / El] + off), m.row_bytes);
          if (PULL) src[k] = make_rsrc(uniform_ptr(s_y[e / El] + off), m.row_bytes);
          if (scaled) w[k] = __uint_as_float((uint32_t)uni((int)__float_as_uint(m.weights[f])));
        }
      }
    }
    const u32x4* g = reinterpret_cast<const u32x4*>(a.in + (uint64_t)t * m.row_bytes);
    for (uint32_t v0 = lane; v0 < nv; v0 += 64 * U) {
      u32x4 d[U];
      u32x4 y[U][kMoeMaxTopK];
#pragma unroll
      for (int u = 0; u < U; ++u)
        if (v0 + u * 64 < nv) d[u] = g[v0 + u * 64];
      if (PULL) {
        // every slot's (peer) load in flight before the first use
#pragma unroll
        for (int k = 0; k < kMoeMaxTopK; ++k) {
          if (on[k]) {
#pragma unroll
            for (int u = 0; u < U; ++u)
              if (v0 + u * 64 < nv) y[u][k] = ld16(src[k], (v0 + u * 64) * 16);
          }
        }
      }
      // push: dy row = w * dout[t], one fp32 multiply and one rounding (a copy without weights)
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (v0 + u * 64 < nv) {
          float dv[R::N];
          R::unpack(d[u], dv);
#pragma unroll
          for (int k = 0; k < kMoeMaxTopK; ++k) {
            if (on[k]) {
              u32x4 o = d[u];
              if (scaled) {
                float sv[R::N];
#pragma unroll
                for (int i = 0; i < R::N; ++i) sv[i] = w[k] * dv[i];
                o = R::pack(sv);
              }
              st16(dst[k], (v0 + u * 64) * 16, o);
            }
          }
          if (PULL) {
            // pull: per-lane fp32 dot in vector order
#pragma unroll
            for (int k = 0; k < kMoeMaxTopK; ++k) {
              if (on[k]) {
                float yv[R::N];
                R::unpack(y[u][k], yv);
#pragma unroll
                for (int i = 0; i < R::N; ++i) dot[k] = __builtin_fmaf(dv[i], yv[i], dot[k]);
              }
            }
          }
        }
      }
    }
    if (PULL) {
#pragma unroll
      for (int k = 0; k < kMoeMaxTopK; ++k) {
        if (k < K) {
          const float s = on[k] ? wave_sum(dot[k]) : 0.0f;
          if (lane == 0) m.dweights[(int64_t)t * K + k] = s;
        }
      }
    }
  }
  if (!sync_phase(a, 3, e0)) return;
  finish(a, e0);
}

}  // namespace

void launch_moe_route(const MoEArgs& m, hipStream_t s) {
  const int nchunks = moe_chunks((int64_t)m.T * m.K);
  if (nchunks) hipLaunchKernelGGL(k_moe_hist, dim3(nchunks), dim3(kThreads), 0, s, m);
  hipLaunchKernelGGL(k_moe_rank, dim3(nchunks ? nchunks : 1), dim3(kThreads), 0, s, m, nchunks);
}

void launch_moe_dispatch(const MoEArgs& m, int grid, hipStream_t s) {
  hipLaunchKernelGGL(k_moe_dispatch, dim3(grid), dim3(kThreads), 0, s, m);
}

void launch_moe_combine(const MoEArgs& m, int grid, hipStream_t s) {
  switch (m.dtype) {
    case DT_F32: hipLaunchKernelGGL(k_moe_combine<DT_F32>, dim3(grid), dim3(kThreads), 0, s, m); break;
    case DT_BF16: hipLaunchKernelGGL(k_moe_combine<DT_BF16>, dim3(grid), dim3(kThreads), 0, s, m); break;
    case DT_F16: hipLaunchKernelGGL(k_moe_combine<DT_F16>, dim3(grid), dim3(kThreads), 0, s, m); break;
    default: throw std::invalid_argument("ccmpi: moe_combine supports bf16, fp16 and fp32");
  }
}

template <int DT>
static void launch_moe_combine_bwd_dt(const MoEArgs& m, int grid, hipStream_t s) {
  if (m.dweights) hipLaunchKernelGGL((k_moe_combine_bwd<DT, true>), dim3(grid), dim3(kThreads), 0, s, m);
  else hipLaunchKernelGGL((k_moe_combine_bwd<DT, false>), dim3(grid), dim3(kThreads), 0, s, m);
}

void launch_moe_combine_bwd(const MoEArgs& m, int grid, hipStream_t s) {
  switch (m.dtype) {
    case DT_F32: launch_moe_combine_bwd_dt<DT_F32>(m, grid, s); break;
    case DT_BF16: launch_moe_combine_bwd_dt<DT_BF16>(m, grid, s); break;
    case DT_F16: launch_moe_combine_bwd_dt<DT_F16>(m, grid, s); break;
    default: throw std::invalid_argument("ccmpi: moe_combine_backward supports bf16, fp16 and fp32");
  }
}

}  // namespace dev
}  // namespace ccmpi
