// Grouped bf16 GEMM over the routed rows of an MoE layer: the experts of one rank
// applied to the buffer moe_dispatch fills, forward and backward, with the row
// counts read from device memory.
//
//   forward  out[r, :] = alpha * x[r, :] . w[g]^T (+ bias[g])   for the rows r of expert g
//            (+ glu[r, j] = silu(out[r, 2j]) * out[r, 2j + 1] from the same epilogue)
//   dX       out[r, :] = alpha * dy[r, :] . w[g]                 for the rows r of expert g
//   wgrad    dw[g]     = alpha * dy[rows of g]^T . x[rows of g]  (fp32)
//
// Expert g owns rows [off_g, off_g + c_g) of the [cap, *] buffers, off_g the prefix
// sum of c_g = max(counts[g], 0); the ranges are clamped to cap (counts that add up
// to more than cap truncate the last experts), so no row at or past cap is read or
// written, and rows at or past sum(c_g) are left untouched.
//
// No kernel's grid depends on the counts.  The forward (and dX, over its K columns) launches
// (ceil(cap / 128) + G) * ceil(N / 128) workgroups, an upper bound on the
// sum_g ceil(c_g / 128) row tiles times the column tiles; every workgroup scans the
// (at most 256) counts at its top -- two block-wide prefix sums, rows then tiles --
// to find its (expert, row tile); the workgroups past the number of real tiles return.  Row
// tiles start at off_g, not at multiples of 128 of the buffer, so a tile never spans
// two experts; its last rows are masked in the store.  The weight gradient launches
// G * ceil(N / 128) * ceil(K / 128) workgroups; each walks its expert's rows in
// order (no split-K, no atomics: deterministic, independent of the other experts).
//
// The tile is the 128x128, BK = 64 v_mfma_f32_16x16x32_bf16 tile of gemm_tile128.hpp,
// the same code the dense kernels of gemm.hip run: LDS-DMA staging with the
// swapped-operand direct epilogue when K % 64 == 0, the register-staged loop with a
// zero-filled K tail otherwise (same LDS image, same epilogue); dX reads w[g] as it lies,
// the reduction over its rows (nn_loop: A staged as in the forward, B in the TN image and
// read through ds_read_b64_tr_b16, its mask a buffer resource over w[g]); the weight gradient is
// the two-tiles-in-flight TN loop over buffer resources that span exactly the expert's
// rows, so rows past its end load as zero.  The kernels here are what is the experts'
// own: the counts, the tile search, the grids and the per-expert operand extents.
#include <pybind11/pybind11.h>

#include <algorithm>
#include <stdexcept>
#include <string>

#include "common.hpp"
#include "gemm_common.hpp"
#include "gemm_tile128.hpp"
#include "ops.hpp"

namespace ccmpi {
namespace dev {

namespace {
using namespace gemm;

constexpr int kMaxGroups = 256;  // = MOE_MAX_EXPERTS (one count per thread of the scan)

struct GroupedArgs {
  const uint16_t* A;    // forward: x [cap, K]; dX, wgrad: dy [cap, N]
  const uint16_t* B;    // forward, dX: w [G][N][K] (strides ldb, b_stride); wgrad: x [cap, K]
  void* C;              // forward: out [cap, N]; dX: out [cap, K]; wgrad: dw [G][N][K] fp32 (strides ldc, c_stride)
  const void* bias;     // forward: [G][N] (row stride bias_ld)
  const void* counts;   // [G] int32 / int64
  int cap, N, K, G;
  int lda, ldb, ldc, bias_ld;
  long long b_stride, c_stride;  // elements between experts
  float alpha;
  int bias_kind;        // 0 none, 1 fp32, 2 bf16
  int counts64;
  void* glu = nullptr;  // forward with the gate: [cap, N / 2] bf16 (row stride ldg)
  int ldg = 0;
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

// The tile search both row-tiled kernels (forward, dX) start with.  The grid is
// (ceil(cap / BM) + G) * tiles_n workgroups; this finds the workgroup's expert g, the first
// row bm of its tile, the end row_end of the expert's rows and its first column bn, or
// returns false (workgroup-uniformly) for a workgroup past the last real tile.
// ws: 4 LDS words, seg: 4 LDS ints.
__device__ __forceinline__ bool find_row_tile(const GroupedArgs& a, int tiles_n, long long* ws, int* seg, int t, int& g,
                                              int& bm, int& row_end, int& bn) {
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
  if ((int)blockIdx.x >= nreal) return false;  // past the last real tile
  const int wg = xcd_remap(blockIdx.x, nreal);
  const int tile = wg / tiles_n;
  bn = (wg % tiles_n) * BN;
  if (tile >= tincl - nt && tile < tincl) {
    seg[0] = t;
    seg[1] = off + (int)(tile - (tincl - nt)) * BM;
    seg[2] = end;
  }
  __syncthreads();
  g = __builtin_amdgcn_readfirstlane(seg[0]);
  if (g < 0) return false;
  bm = __builtin_amdgcn_readfirstlane(seg[1]);
  row_end = __builtin_amdgcn_readfirstlane(seg[2]);
  return true;
}

// ---------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------
// GLU (bf16 out): a.glu [cap, N / 2] gets the SwiGLU gate of the output's (gate, up) column
// pairs from the same epilogue, for the same rows.
template <bool GLDS, bool OUT_BF16, bool GLU>
__global__ void __launch_bounds__(NT) k_grouped_gemm_nt(GroupedArgs a) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[kNtLoopBytes];
  __shared__ long long ws[4];
  __shared__ int seg[4];  // expert, first row of the tile, end of the expert's rows; row tiles in all
  const int t = threadIdx.x, lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  int g, bm, row_end, bn;
  if (!find_row_tile(a, (a.N + BN - 1) / BN, ws, seg, t, g, bm, row_end, bn)) return;
  const uint16_t* Bg = a.B + (size_t)g * a.b_stride;

  // Rows past the expert's end / past N are re-read (LDS-DMA) or zero-filled (register
  // staging, with the K tail) by the shared loops and masked in the store, so nothing
  // outside the expert's rows is touched.  Both loops stage B pair-permuted and swap the
  // MFMA operands for the direct epilogue.
  floatx4 acc[4][4];
  const NtSrc src{a.A, Bg, a.lda, a.ldb, bm, row_end, bn, a.N, a.K, 0, GLDS ? a.K / BK : (a.K + BK - 1) / BK};
  if constexpr (GLDS) nt_loop_glds(src, smem, acc, wave, lane);
  else nt_loop_regs<true>(src, smem, acc, wave, t);

  const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64;
  const void* bias = nullptr;  // bias[g]
  if (a.bias_kind) bias = reinterpret_cast<const char*>(a.bias) + (size_t)g * a.bias_ld * (a.bias_kind == 1 ? 4 : 2);
  const TileDst dst{a.C, a.ldc, row_end, a.N, a.alpha, bias, a.bias_kind, a.glu, a.ldg};
  store_direct_fast<OUT_BF16, GLU>(dst, acc, bm + wm, bn + wn, lane);
}

// ---------------------------------------------------------------------------
// dX: out[r, :] = alpha * dy[r, :] . w[g] for the rows r of expert g, w[g] [N, K] read as it
// lies (the reduction over its rows): nn_loop, the forward's tile search and row rules.
// a.A = dy [cap, N], a.B = w, a.C = out [cap, K]; the reduction is a.N, the columns a.K.
// ---------------------------------------------------------------------------
template <bool GLDS, bool OUT_BF16>
__global__ void __launch_bounds__(NT) k_grouped_gemm_nn(GroupedArgs a) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[kNnLoopBytes];
  __shared__ long long ws[4];
  __shared__ int seg[4];
  const int t = threadIdx.x, lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  int g, bm, row_end, bn;
  if (!find_row_tile(a, (a.K + BN - 1) / BN, ws, seg, t, g, bm, row_end, bn)) return;
  // The mask of B is its buffer resource: w[g]'s N rows, ending with the last element of the
  // last one, so the reduction tail past N (the next expert's weights, or the end of the
  // allocation) loads as zero; dy's side of the tail is zero-filled by the loop.
  const uint16_t* Bg = a.B + (size_t)g * a.b_stride;
  const uint32_t bytes_b = (uint32_t)(((size_t)(a.N - 1) * a.ldb + a.K) * 2);
  const Rsrc rsb = make_rsrc(uniform_ptr(reinterpret_cast<char*>(const_cast<uint16_t*>(Bg))), bytes_b);

  floatx4 acc[4][4];
  const NtSrc src{a.A, nullptr, a.lda, a.ldb, bm, row_end, bn, 0, a.N, 0, GLDS ? a.N / BK : (a.N + BK - 1) / BK};
  nn_loop<GLDS>(src, rsb, smem, acc, wave, t);

  const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64;
  const TileDst dst{a.C, a.ldc, row_end, a.K, a.alpha, nullptr, 0};
  store_direct4<OUT_BF16>(dst, acc, bm + wm, bn + wn, lane);
}

// ---------------------------------------------------------------------------
// weight gradient: dw[g][N][K] = alpha * dy[rows of g]^T . x[rows of g]
// (tn_loop_pf2: 64-row tiles of both operands staged as they are, MFMA operands
// through ds_read_b64_tr_b16, two tiles in flight in two register sets)
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(2))) k_grouped_gemm_tn(GroupedArgs a) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[4 * kTnTile];
  __shared__ long long ws[4];
  __shared__ int seg[2];
  const int t = threadIdx.x;
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

  floatx4 acc[4][4];
  // The mask is the buffer resource: it starts at the expert's first row and ends with the
  // last element of its last row, so rows past the expert's end (the next expert's, spare
  // rows, whatever they hold) load as zero and contribute exactly nothing.  Columns past
  // N / K read the row's neighbours inside the expert, or zero on its last row; they only
  // reach outputs that are never stored.
  const uint16_t* Ag = a.A + (size_t)off * a.lda;
  const uint16_t* Bg = a.B + (size_t)off * a.ldb;
  const uint32_t bytes_a = rows > 0 ? (uint32_t)(((size_t)(rows - 1) * a.lda + a.N) * 2) : 0u;
  const uint32_t bytes_b = rows > 0 ? (uint32_t)(((size_t)(rows - 1) * a.ldb + a.K) * 2) : 0u;
  const Rsrc rsa = make_rsrc(uniform_ptr(reinterpret_cast<char*>(const_cast<uint16_t*>(Ag))), bytes_a);
  const Rsrc rsb = make_rsrc(uniform_ptr(reinterpret_cast<char*>(const_cast<uint16_t*>(Bg))), bytes_b);
  tn_loop_pf2(rsa, rsb, a.lda, a.ldb, bm, bn, (rows + BK - 1) / BK, smem, acc, t);
  __syncthreads();
  // LDS-staged fp32 rows (the operand buffers are dead): an expert with no rows stores zeros
  float* Cg = reinterpret_cast<float*>(a.C) + (size_t)g * a.c_stride;
  store_tile_f32<false, false>(TileDst{Cg, a.ldc, a.N, a.K, a.alpha, nullptr, 0}, acc, smem, bm, bn, t);
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

// glu != 0 (bf16 out only): the forward with the SwiGLU gate in its epilogue
void launch_grouped_nt(const char* op, uint64_t X, uint64_t W, uint64_t Out, uint64_t glu, uint64_t bias,
                       uint64_t counts, int cap, int N, int K, int G, int ldx, int ldw, long long w_stride, int ldo,
                       int ldg, int bias_ld, float alpha, int bias_kind, bool out_bf16, bool counts64, uint64_t stream) {
  const std::string who = std::string("ccmpi ") + op + ": ";
  check_common(op, X, W, Out, counts, cap, N, K, G, ldx, ldw);
  if (w_stride % 8 || (ldo * (out_bf16 ? 2 : 4)) % 16 || bias_kind < 0 || bias_kind > 2 || (bias_kind && bias == 0))
    throw std::invalid_argument(who + "16-B aligned expert stride and output rows, bias kind 0..2");
  if (glu && (!out_bf16 || glu % 8 || ldg % 4 || ldg < N / 2))
    throw std::invalid_argument(who + "the gate needs a bf16 output and 8-B aligned glu rows of at least N / 2");
  if (cap <= 0) return;
  const long long row_tiles = (cap + BM - 1) / BM + G, grid = row_tiles * ((N + BN - 1) / BN);
  if (grid >= (1ll << 31)) throw std::invalid_argument(who + "grid too large");
  GroupedArgs a{reinterpret_cast<const uint16_t*>(X), reinterpret_cast<const uint16_t*>(W), reinterpret_cast<void*>(Out),
                reinterpret_cast<const void*>(bias), reinterpret_cast<const void*>(counts), cap, N, K, G, ldx, ldw, ldo,
                bias_ld, w_stride, 0, alpha, bias_kind, counts64 ? 1 : 0, reinterpret_cast<void*>(glu), ldg};
  auto st = reinterpret_cast<hipStream_t>(stream);
  const dim3 gr((unsigned)grid), bl(NT);
  if (K % BK == 0) {
    if (glu) hipLaunchKernelGGL((k_grouped_gemm_nt<true, true, true>), gr, bl, 0, st, a);
    else if (out_bf16) hipLaunchKernelGGL((k_grouped_gemm_nt<true, true, false>), gr, bl, 0, st, a);
    else hipLaunchKernelGGL((k_grouped_gemm_nt<true, false, false>), gr, bl, 0, st, a);
  } else {
    if (glu) hipLaunchKernelGGL((k_grouped_gemm_nt<false, true, true>), gr, bl, 0, st, a);
    else if (out_bf16) hipLaunchKernelGGL((k_grouped_gemm_nt<false, true, false>), gr, bl, 0, st, a);
    else hipLaunchKernelGGL((k_grouped_gemm_nt<false, false, false>), gr, bl, 0, st, a);
  }
  CCMPI_HIP_CHECK(hipGetLastError());
}

void grouped_gemm_nt(uint64_t X, uint64_t W, uint64_t Out, uint64_t bias, uint64_t counts, int cap, int N, int K,
                     int G, int ldx, int ldw, long long w_stride, int ldo, int bias_ld, float alpha, int bias_kind,
                     bool out_bf16, bool counts64, uint64_t stream) {
  launch_grouped_nt("grouped_gemm_nt", X, W, Out, 0, bias, counts, cap, N, K, G, ldx, ldw, w_stride, ldo, 0, bias_ld,
                    alpha, bias_kind, out_bf16, counts64, stream);
}

void grouped_gemm_nt_swiglu(uint64_t X, uint64_t W, uint64_t H, uint64_t Glu, uint64_t bias, uint64_t counts, int cap,
                            int N, int K, int G, int ldx, int ldw, long long w_stride, int ldh, int ldg, int bias_ld,
                            float alpha, int bias_kind, bool counts64, uint64_t stream) {
  if (cap > 0 && Glu == 0) throw std::invalid_argument("ccmpi grouped_gemm_nt_swiglu: null operand");
  launch_grouped_nt("grouped_gemm_nt_swiglu", X, W, H, Glu, bias, counts, cap, N, K, G, ldx, ldw, w_stride, ldh, ldg,
                    bias_ld, alpha, bias_kind, true, counts64, stream);
}

// dy [cap, N] . w[g] [N, K] -> out [cap, K]
void grouped_gemm_nn(uint64_t dY, uint64_t W, uint64_t Out, uint64_t counts, int cap, int N, int K, int G, int lddy,
                     int ldw, long long w_stride, int ldo, float alpha, bool out_bf16, bool counts64, uint64_t stream) {
  check_common("grouped_gemm_nn", dY, W, Out, counts, cap, N, K, G, lddy, ldw);
  if (w_stride % 8 || (ldo * (out_bf16 ? 2 : 4)) % 16 || ldw < K)
    throw std::invalid_argument("ccmpi grouped_gemm_nn: 16-B aligned expert stride and output rows, row stride >= K");
  // one expert's weights are addressed with 32-bit byte offsets from its first row; the
  // offsets of the reduction tail's rows and of the last column tile (all masked) must not wrap
  if (((size_t)N + BK) * (size_t)ldw * 2 + ((size_t)K + BN) * 2 >= (1ull << 31))
    throw std::invalid_argument("ccmpi grouped_gemm_nn: one expert's weights (N * row stride) must stay below 2 GiB");
  if (cap <= 0) return;
  const long long row_tiles = (cap + BM - 1) / BM + G, grid = row_tiles * ((K + BN - 1) / BN);
  if (grid >= (1ll << 31)) throw std::invalid_argument("ccmpi grouped_gemm_nn: grid too large");
  GroupedArgs a{reinterpret_cast<const uint16_t*>(dY), reinterpret_cast<const uint16_t*>(W), reinterpret_cast<void*>(Out),
                nullptr, reinterpret_cast<const void*>(counts), cap, N, K, G, lddy, ldw, ldo, 0, w_stride, 0, alpha, 0,
                counts64 ? 1 : 0};
  auto st = reinterpret_cast<hipStream_t>(stream);
  const dim3 gr((unsigned)grid), bl(NT);
  if (N % BK == 0) {
    if (out_bf16) hipLaunchKernelGGL((k_grouped_gemm_nn<true, true>), gr, bl, 0, st, a);
    else hipLaunchKernelGGL((k_grouped_gemm_nn<true, false>), gr, bl, 0, st, a);
  } else {
    if (out_bf16) hipLaunchKernelGGL((k_grouped_gemm_nn<false, true>), gr, bl, 0, st, a);
    else hipLaunchKernelGGL((k_grouped_gemm_nn<false, false>), gr, bl, 0, st, a);
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
  m.def("grouped_gemm_nt_swiglu", &grouped_gemm_nt_swiglu,
        "h = grouped_gemm_nt(x, w) in bf16 and glu[r, j] = silu(h[r, 2j]) * h[r, 2j + 1], one kernel",
        pybind11::arg("x"), pybind11::arg("w"), pybind11::arg("h"), pybind11::arg("glu"), pybind11::arg("bias"),
        pybind11::arg("counts"), pybind11::arg("cap"), pybind11::arg("N"), pybind11::arg("K"), pybind11::arg("G"),
        pybind11::arg("ldx"), pybind11::arg("ldw"), pybind11::arg("w_stride"), pybind11::arg("ldh"),
        pybind11::arg("ldg"), pybind11::arg("bias_ld"), pybind11::arg("alpha"), pybind11::arg("bias_kind"),
        pybind11::arg("counts64"), pybind11::arg("stream"), pybind11::call_guard<pybind11::gil_scoped_release>());
  m.def("grouped_gemm_nn", &grouped_gemm_nn,
        "out[rows of g] = alpha * dy[rows of g] . w[g] (w [G][N][K] as the forward takes it); counts on the device",
        pybind11::arg("dy"), pybind11::arg("w"), pybind11::arg("out"), pybind11::arg("counts"), pybind11::arg("cap"),
        pybind11::arg("N"), pybind11::arg("K"), pybind11::arg("G"), pybind11::arg("lddy"), pybind11::arg("ldw"),
        pybind11::arg("w_stride"), pybind11::arg("ldo"), pybind11::arg("alpha"), pybind11::arg("out_bf16"),
        pybind11::arg("counts64"), pybind11::arg("stream"), pybind11::call_guard<pybind11::gil_scoped_release>());
  m.def("grouped_gemm_tn", &grouped_gemm_tn,
        "dw[g][N][K] = alpha * dy[rows of g]^T . x[rows of g] (fp32); the rows per expert read from device counts",
        pybind11::arg("dy"), pybind11::arg("x"), pybind11::arg("dw"), pybind11::arg("counts"), pybind11::arg("cap"),
        pybind11::arg("N"), pybind11::arg("K"), pybind11::arg("G"), pybind11::arg("lddy"), pybind11::arg("ldx"),
        pybind11::arg("lddw"), pybind11::arg("dw_stride"), pybind11::arg("alpha"), pybind11::arg("counts64"),
        pybind11::arg("stream"), pybind11::call_guard<pybind11::gil_scoped_release>());
}

}  // namespace dev
}  // namespace ccmpi
