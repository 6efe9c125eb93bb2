// The 128x128, BK = 64 v_mfma_f32_16x16x32_bf16 workgroup tile shared by the dense
// kernels (gemm.hip) and the grouped expert kernels (grouped_gemm.hip): main loops
// and the value-described epilogues, each defined once.  256 threads, 4 waves as
// 2x2, each wave 64x64 = 4x4 MFMA tiles.  A kernel is a prologue that finds its
// tile, one of the loops below, and an epilogue (TileDst, or the GemmArgs epilogues
// that stay in gemm.hip).  Nothing here knows which kernel calls it: what differs
// between the callers are the values they pass (NtSrc, TileDst, plain arguments).
#pragma once
#include <cstdint>

#include "common.hpp"
#include "gemm_common.hpp"

namespace ccmpi {
namespace dev {
namespace gemm {

constexpr int BM = 128, BN = 128, BK = 64, NT = 256;
constexpr int kRowBytes = BK * 2;                         // 128 B per LDS row (NT loops)
constexpr int kNtLoopBytes = 2 * (BM + BN) * kRowBytes;   // two A + B buffers of the NT loops
constexpr int kEpiBytes = BM * (BN + 4) * 4;              // fp32 tile of the LDS-staged epilogues
typedef short v4s __attribute__((ext_vector_type(4)));
typedef short v8s __attribute__((ext_vector_type(8)));
constexpr int kTnRow = 288;             // TN loop: bytes per LDS row (256 data + 32 pad)
constexpr int kTnTile = BK * kTnRow;    // one operand tile

// What one workgroup of an NT loop reads: A rows bm.. (valid below a_end) and B rows
// bn.. (valid below b_end), both K-contiguous, over K tiles kt0 .. kt0 + nk - 1.
struct NtSrc {
  const uint16_t* A;
  const uint16_t* B;
  int lda, ldb;
  int bm, a_end;
  int bn, b_end;
  int K;        // reduction length: the register-staged loop zero-fills past it
  int kt0, nk;  // first K tile (of BK) and the number of tiles to walk
};

// Where the tile goes: rows below row_end and columns below col_end are stored.
struct TileDst {
  void* C;
  int ldc;
  int row_end, col_end;
  float alpha;
  const void* bias;  // [col_end] fp32 / bf16, null without a bias
  int bias_kind;     // 0 none, 1 fp32, 2 bf16
  void* glu = nullptr;  // store_direct_fast<true, true>: [row_end][col_end / 2] bf16 SwiGLU gate of C's column pairs
  int ldg = 0;
};

__device__ __forceinline__ void zero_acc(floatx4 (&acc)[4][4]) {
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = floatx4{0.f, 0.f, 0.f, 0.f};
}

// The direct (LDS-free) epilogues are for loops that swap the MFMA operands and stage
// B rows in the "pair" permutation: LDS row 32p + 16h + q of the B tile holds
// output column 32p + 8*(q >> 2) + 4h + (q & 3).  The accumulator of tile
// (i, j = 2p + h) then holds C[row0 + 16i + (lane & 15)][col0 + 32p + 8*(lane >> 4) + 4h + r],
// i.e. 8 consecutive columns of one row per lane and pair: one 16-B vector store
// (bf16) or two (fp32).
__device__ __forceinline__ int pair_perm(int r) {
  return (r & ~31) | (((r & 15) >> 2) << 3) | (((r >> 4) & 1) << 2) | (r & 3);
}

// ---------------------------------------------------------------------------
// NT loops: acc = A[bm.., K range] . B[bn.., K range]^T.  Two LDS buffers of
// (BM + BN) rows of 128 B; the 16-B chunk index is XOR-swizzled with (row & 7)
// so a 16-lane ds_read_b128 group touches 8 different slots.
// DIRECT: pair-permuted B rows and swapped MFMA operands (for the direct epilogues).
// ---------------------------------------------------------------------------
__device__ __forceinline__ unsigned char* nt_as(unsigned char* smem, int buf) { return smem + buf * ((BM + BN) * kRowBytes); }
__device__ __forceinline__ unsigned char* nt_bs(unsigned char* smem, int buf) { return nt_as(smem, buf) + BM * kRowBytes; }

// Per-lane byte offsets, inside one LDS buffer, of the wave's first A / B fragment row for
// the two 32-deep k-steps of a staged K tile: row wm + (lane & 15) resp. BM + wn + (lane & 15),
// chunk ks * 4 + (lane >> 4) swizzled with (row & 7) = (lane & 7) (wm, wn and 16 i are
// multiples of 8).  Computed once before the loop, so a K step spends one add per offset
// before its first fragment read; fragment i is 16 i rows (an immediate) further.
struct NtFragOff {
  int a[2], b[2];
};
__device__ __forceinline__ NtFragOff nt_frag_off(int wm, int wn, int lane) {
  NtFragOff o;
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) {
    const int sw = ((ks * 4 + (lane >> 4)) ^ (lane & 7)) << 4;
    o.a[ks] = (wm + (lane & 15)) * kRowBytes + sw;
    o.b[ks] = (BM + wn + (lane & 15)) * kRowBytes + sw;
  }
  return o;
}

// every fragment of the staged K tile in buffer `buf` (= nt_as(smem, cur)): the wave's 64
// rows of A and of B, both k-steps
__device__ __forceinline__ void nt_read_frags(const unsigned char* buf, const NtFragOff& o, bf16x8 (&af)[2][4],
                                              bf16x8 (&bf)[2][4]) {
#pragma unroll
  for (int ks = 0; ks < 2; ++ks)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      af[ks][i] = *reinterpret_cast<const bf16x8*>(buf + o.a[ks] + i * 16 * kRowBytes);
      bf[ks][i] = *reinterpret_cast<const bf16x8*>(buf + o.b[ks] + i * 16 * kRowBytes);
    }
}

// the MFMAs of one staged K tile; DIRECT: operands swapped (B rows first)
template <bool DIRECT>
__device__ __forceinline__ void nt_mfmas(const bf16x8 (&af)[2][4], const bf16x8 (&bf)[2][4], floatx4 (&acc)[4][4]) {
#pragma unroll
  for (int ks = 0; ks < 2; ++ks)
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if constexpr (DIRECT) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bf[ks][j], af[ks][i], acc[i][j], 0, 0, 0);
        else acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[ks][i], bf[ks][j], acc[i][j], 0, 0, 0);
      }
}

// Staged by LDS-DMA (global_load_lds, 16 B per lane, 1 KiB per wave instruction)
// instead of registers: the next K-tile streams straight into the other LDS buffer
// while this one feeds the MFMAs, and the staging costs no VGPRs and no ds_write
// issue slots.  The LDS image is lane-linear (8 rows of 128 B per instruction), so
// the (row & 7) chunk swizzle the fragment reads expect is applied to the per-lane
// SOURCE address (the same involution on both sides).  Rows past a_end / b_end
// re-read the last valid row (their outputs are discarded, and nothing outside the
// valid rows is touched); only for K % 64 == 0.  `wave` must be wave-uniform.  Always the
// DIRECT form (swapped MFMA operands, pair-permuted B rows; nt_mfmas).
__device__ __forceinline__ void nt_loop_glds(const NtSrc& s, unsigned char* smem, floatx4 (&acc)[4][4], int wave,
                                             int lane) {
  const NtFragOff fo = nt_frag_off((wave >> 1) * 64, (wave & 1) * 64, lane);
  // per-lane source row / swizzled chunk for the 4 instructions of this wave
  const int lrow = lane >> 3, pchunk = lane & 7;
  auto issue = [&](int k0, int buf) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int q = wave * 4 + i;                 // 1 KiB LDS chunk = rows q*8 .. q*8+7
      const int r = q * 8 + lrow;
      const int c = pchunk ^ (r & 7);             // logical k-chunk this lane must fetch
      const int ga = min(s.bm + r, s.a_end - 1), gb = min(s.bn + pair_perm(r), s.b_end - 1);
      __builtin_amdgcn_global_load_lds((const void*)(s.A + (size_t)ga * s.lda + k0 + c * 8),
                                       (__attribute__((address_space(3))) void*)(nt_as(smem, buf) + q * 1024), 16, 0, 0);
      __builtin_amdgcn_global_load_lds((const void*)(s.B + (size_t)gb * s.ldb + k0 + c * 8),
                                       (__attribute__((address_space(3))) void*)(nt_bs(smem, buf) + q * 1024), 16, 0, 0);
    }
  };
  // An empty K range (a split past the end of K) leaves before the wait and the barrier,
  // workgroup-uniformly.  Written as `if (nk > 0) issue(...)` in front of one zero_acc, the
  // compiler schedules the 64 accumulator writes between the DMA wait and the barrier and
  // once more after it; in this form they are interleaved with the first tile's DMA issue
  // (profiles/gemm_tile128/README.md, "The prologue of the LDS-DMA loop").
  if (s.nk <= 0) {
    zero_acc(acc);
    return;
  }
  issue(s.kt0 * BK, 0);
  zero_acc(acc);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  for (int kt = 0; kt < s.nk; ++kt) {
    const int cur = kt & 1;
    // all fragment reads of this K-tile BEFORE the next tile's DMA is issued:
    // the compiler cannot prove the DMA target disjoint from the reads and
    // would otherwise wait for the DMA before the remaining ds_reads
    bf16x8 af[2][4], bf[2][4];
    nt_read_frags(nt_as(smem, cur), fo, af, bf);
    if (kt + 1 < s.nk) issue((s.kt0 + kt + 1) * BK, cur ^ 1);
    __builtin_amdgcn_s_setprio(1);
    nt_mfmas<true>(af, bf, acc);
    __builtin_amdgcn_s_setprio(0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }
}

// Staged through registers, for any K % 8 == 0: global -> register loads of tile
// k+1 are issued before the MFMAs of tile k and written to the other LDS buffer
// after them (one barrier per K-step).  Same LDS image as the LDS-DMA loop; rows
// past a_end / b_end and the K tail are zero-filled.
template <bool DIRECT>
__device__ __forceinline__ void nt_loop_regs(const NtSrc& s, unsigned char* smem, floatx4 (&acc)[4][4], int wave,
                                             int t) {
  zero_acc(acc);
  const NtFragOff fo = nt_frag_off((wave >> 1) * 64, (wave & 1) * 64, t & 63);
  uint4 ra[4], rb[4];
  const int srow = t >> 3, schunk = t & 7;
  auto gload = [&](int k0) {
    const int gk = k0 + schunk * 8;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r = srow + 32 * i;
      const int gm = s.bm + r, gn = s.bn + (DIRECT ? pair_perm(r) : r);
      ra[i] = (gm < s.a_end && gk < s.K) ? *reinterpret_cast<const uint4*>(s.A + (size_t)gm * s.lda + gk) : uint4{0, 0, 0, 0};
      rb[i] = (gn < s.b_end && gk < s.K) ? *reinterpret_cast<const uint4*>(s.B + (size_t)gn * s.ldb + gk) : uint4{0, 0, 0, 0};
    }
  };
  auto swrite = [&](int buf) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r = srow + 32 * i;
      const int off = r * kRowBytes + ((schunk ^ (r & 7)) << 4);
      *reinterpret_cast<uint4*>(nt_as(smem, buf) + off) = ra[i];
      *reinterpret_cast<uint4*>(nt_bs(smem, buf) + off) = rb[i];
    }
  };
  if (s.nk > 0) {
    gload(s.kt0 * BK);
    swrite(0);
  }
  __syncthreads();
  for (int kt = 0; kt < s.nk; ++kt) {
    const int cur = kt & 1;
    if (kt + 1 < s.nk) gload((s.kt0 + kt + 1) * BK);
    bf16x8 af[2][4], bf[2][4];
    nt_read_frags(nt_as(smem, cur), fo, af, bf);
    nt_mfmas<DIRECT>(af, bf, acc);
    if (kt + 1 < s.nk) swrite(cur ^ 1);
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------
// TN tile: acc = A[K range, bm..]^T . B[K range, bn..], A and B row-major with
// the reduction over their rows.  Tiles of 64 rows x 128 columns are staged
// as-is into LDS; MFMA operands (8 consecutive rows for one column per lane)
// come out of gfx950's transposing LDS read ds_read_b64_tr_b16, two reads per
// operand per 32-deep k-step.  LDS rows are 256 B + 32 B pad (row r starts 8
// banks after row r-1) and the two 128-B halves of rows with bit 3 set are
// swapped, so every tr read (a 32-lane half spans rows r..r+3 and r+8..r+11)
// is bank-conflict free.
// ---------------------------------------------------------------------------
__device__ __forceinline__ int tn_off(int row, int byte) { return row * kTnRow + (byte ^ (((row >> 3) & 1) << 7)); }

__device__ __forceinline__ unsigned char* tn_as(unsigned char* smem, int buf) { return smem + buf * (2 * kTnTile); }
__device__ __forceinline__ unsigned char* tn_bs(unsigned char* smem, int buf) { return tn_as(smem, buf) + kTnTile; }

// one K tile held in registers (thread t: rows (t >> 4) + 16 i, 16-B chunk t & 15 of the
// 128 columns) -> LDS buffer buf
__device__ __forceinline__ void tn_stage(unsigned char* smem, int buf, const uint4 (&ra)[4], const uint4 (&rb)[4], int t) {
  const int schunk = t & 15, srow = t >> 4;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int r = srow + 16 * i;
    *reinterpret_cast<uint4*>(tn_as(smem, buf) + tn_off(r, schunk * 16)) = ra[i];
    *reinterpret_cast<uint4*>(tn_bs(smem, buf) + tn_off(r, schunk * 16)) = rb[i];
  }
}

// the MFMAs of the K tile staged in LDS buffer cur
__device__ __forceinline__ void tn_compute(unsigned char* smem, int cur, floatx4 (&acc)[4][4], int t) {
  const int wave = t >> 6, lane = t & 63;
  const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64;
  const int grp = lane >> 4, q = (lane >> 2) & 3, p = lane & 3;
  // fragment read addresses: tn_off(ks * 32 + grp * 8 + q + 4 h, (w + 16 i + 4 p) * 2) is a
  // per-lane base plus the constant ks * 32 * kTnRow + h * 4 * kTnRow + 32 i: the half-swap
  // XOR only flips the 128-B bit that w * 2 (w in {0, 64}) owns (row bit 3 = grp & 1; q + 4h
  // < 8 never carries into it), so every read is base + an immediate offset
  const int lrow = (grp * 8 + q) * kTnRow, xsw = (grp & 1) << 7;
  const int la = lrow + ((wm * 2) ^ xsw) + 8 * p, lb = lrow + ((wn * 2) ^ xsw) + 8 * p;
  const unsigned char* abase = tn_as(smem, cur) + la;
  const unsigned char* bbase = tn_bs(smem, cur) + lb;
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
}

// The two-tiles-in-flight loop over buffer resources, as the grouped weight gradient runs it
// (k_gemm_tn of gemm.hip keeps its own loads and schedule, PF = 1 and 2, around tn_stage and
// tn_compute: moved in here, the compiler formed its load addresses differently and the
// kernel measured up to 1.2 % slower, profiles/gemm_tile128/README.md).  rsa / rsb start at
// the first row of the reduction and end with its last valid element: rows past it read as
// 0 with no branch, so the loads carry no exec-mask control flow and the compiler can wait
// for the older register set alone.  ca / cb: first column of A / B; columns past the
// operand's width read the row's neighbours, which only reach outputs that are never stored.
__device__ __forceinline__ void tn_loop_pf2(Rsrc rsa, Rsrc rsb, int lda, int ldb, int ca, int cb, int nk,
                                            unsigned char* smem, floatx4 (&acc)[4][4], int t) {
  constexpr int PF = 2;
  zero_acc(acc);
  uint4 ra[PF][4], rb[PF][4];
  const int schunk = t & 15, srow = t >> 4;
  auto gload = [&](int set, int j) {  // K tile j -> register set
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const uint32_t m = (uint32_t)(j * BK + srow + 16 * i);
      ra[set][i] = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(rsa.r, (m * lda + ca + schunk * 8) * 2, 0, 0));
      rb[set][i] = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(rsb.r, (m * ldb + cb + schunk * 8) * 2, 0, 0));
    }
  };
  // tile j is loaded into register set j % PF and written to LDS buffer j & 1 one step
  // before its MFMAs; set j % PF is refilled with tile j + PF right after that write
#pragma unroll
  for (int u = 0; u < PF; ++u)
    if (u < nk) gload(u, u);
  if (nk > 0) tn_stage(smem, 0, ra[0], rb[0], t);
  __syncthreads();
  if (PF < nk) gload(0, PF);
  for (int kt = 0; kt < nk; kt += PF) {
#pragma unroll
    for (int u = 0; u < PF; ++u) {
      if (kt + u < nk) {
        tn_compute(smem, u & 1, acc, t);
        if (kt + u + 1 < nk) tn_stage(smem, (u + 1) & 1, ra[(u + 1) % PF], rb[(u + 1) % PF], t);
        __syncthreads();
        if (kt + u + 1 + PF < nk) gload((u + 1) % PF, kt + u + 1 + PF);
      }
    }
  }
}

// ---------------------------------------------------------------------------
// NN loop: acc = A[bm.., reduction range] . B[reduction range, bn..], A contiguous in the
// reduction (as in the NT loops), B row-major with the reduction over its rows (as in the
// TN tile).  A is staged in the NT image (LDS-DMA for GLDS, which needs a reduction length
// that is a multiple of 64; through registers with a zero-filled tail otherwise), B's 64
// reduction rows x 128 columns are staged as they are in the TN image and read through
// ds_read_b64_tr_b16 with tn_compute's addresses.  Both fragments are the standard
// 16x16x32 operand (index lane & 15, reduction elements 8 * (lane >> 4) .. + 7), so they
// meet in one MFMA; the operands are swapped (B first), which leaves every lane 4
// consecutive columns of one row: acc[i][j][r] = C[bm + wm + 16 i + (lane & 15)]
// [bn + wn + 16 j + 4 * (lane >> 4) + r] (store_direct4).
// B is read through the buffer resource rsb, which starts at B's first reduction row and
// ends with the last element of its last one: rows past the reduction load as zero with no
// branch, so whatever lies behind them never reaches an MFMA (A's side of the tail is
// zero-filled too, so the tail is 0 * 0).  Columns past B's width read the row's
// neighbours, which only reach outputs that are never stored.  Every lane runs every
// transposing read (it needs EXEC all ones); only the A loads of the register-staged
// form are predicated.
// ---------------------------------------------------------------------------
constexpr int kNnABytes = BM * kRowBytes;                     // one A buffer (NT image)
constexpr int kNnLoopBytes = 2 * kNnABytes + 2 * kTnTile;     // two A + two B buffers
__device__ __forceinline__ unsigned char* nn_as(unsigned char* smem, int buf) { return smem + buf * kNnABytes; }
__device__ __forceinline__ unsigned char* nn_bs(unsigned char* smem, int buf) { return smem + 2 * kNnABytes + buf * kTnTile; }

// s: A, lda, bm, a_end, K = reduction length, nk = its BK tiles (B, ldb, b_end and kt0 are
// not used: B comes through rsb, row stride ldb elements, first column bn)
template <bool GLDS>
__device__ __forceinline__ void nn_loop(const NtSrc& s, Rsrc rsb, unsigned char* smem, floatx4 (&acc)[4][4], int wave,
                                        int t) {
  const int lane = t & 63;
  const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64;
  const NtFragOff fo = nt_frag_off(wm, wn, lane);
  // B fragment addresses: tn_compute's (bank-conflict free in this pattern only)
  const int grp = lane >> 4, q = (lane >> 2) & 3, p = lane & 3;
  const int lb = (grp * 8 + q) * kTnRow + ((wn * 2) ^ ((grp & 1) << 7)) + 8 * p;
  uint4 ra[GLDS ? 1 : 4], rb[4];
  const int brow = t >> 4, bchunk = t & 15;  // B staging: rows brow + 16 i, 16-B chunk bchunk
  const int arow = t >> 3, achunk = t & 7;   // A register staging: rows arow + 32 i, chunk achunk
  const int lrow = lane >> 3, pchunk = lane & 7;
  auto gload_b = [&](int kt) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const uint32_t n = (uint32_t)(kt * BK + brow + 16 * i);
      rb[i] = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(rsb.r, (n * s.ldb + s.bn + bchunk * 8) * 2, 0, 0));
    }
  };
  auto load_a = [&](int kt, int buf) {
    if constexpr (GLDS) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int c16 = wave * 4 + i;  // 1 KiB LDS chunk = rows c16 * 8 .. + 7
        const int r = c16 * 8 + lrow;
        const int c = pchunk ^ (r & 7);
        const int ga = min(s.bm + r, s.a_end - 1);
        __builtin_amdgcn_global_load_lds((const void*)(s.A + (size_t)ga * s.lda + kt * BK + c * 8),
                                         (__attribute__((address_space(3))) void*)(nn_as(smem, buf) + c16 * 1024), 16, 0, 0);
      }
    } else {
      const int gk = kt * BK + achunk * 8;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int gm = s.bm + arow + 32 * i;
        ra[i] = (gm < s.a_end && gk < s.K) ? *reinterpret_cast<const uint4*>(s.A + (size_t)gm * s.lda + gk) : uint4{0, 0, 0, 0};
      }
    }
  };
  auto swrite = [&](int buf) {
    if constexpr (!GLDS) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int r = arow + 32 * i;
        *reinterpret_cast<uint4*>(nn_as(smem, buf) + r * kRowBytes + ((achunk ^ (r & 7)) << 4)) = ra[i];
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) *reinterpret_cast<uint4*>(nn_bs(smem, buf) + tn_off(brow + 16 * i, bchunk * 16)) = rb[i];
  };
  zero_acc(acc);
  if (s.nk <= 0) return;  // workgroup-uniform
  load_a(0, 0);
  gload_b(0);
  swrite(0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  for (int kt = 0; kt < s.nk; ++kt) {
    const int cur = kt & 1;
    // every fragment read of this tile before the next tile's loads are issued (see nt_loop_glds)
    bf16x8 af[2][4], bf[2][4];
    const unsigned char* abase = nn_as(smem, cur);
    const unsigned char* bbase = nn_bs(smem, cur) + lb;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        af[ks][i] = *reinterpret_cast<const bf16x8*>(abase + fo.a[ks] + i * 16 * kRowBytes);
        const int o = ks * 32 * kTnRow + 32 * i;
        const v4s b0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) v4s*)(bbase + o));
        const v4s b1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) v4s*)(bbase + o + 4 * kTnRow));
        bf[ks][i] = __builtin_bit_cast(bf16x8, (v8s)__builtin_shufflevector(b0, b1, 0, 1, 2, 3, 4, 5, 6, 7));
      }
    if (kt + 1 < s.nk) {
      load_a(kt + 1, cur ^ 1);
      gload_b(kt + 1);
    }
    __builtin_amdgcn_s_setprio(1);
    nt_mfmas<true>(af, bf, acc);
    __builtin_amdgcn_s_setprio(0);
    if (kt + 1 < s.nk) swrite(cur ^ 1);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------
// epilogues on a destination described by values
// ---------------------------------------------------------------------------

// Branch-free direct epilogue (pair_perm above) for the common case: no split-K, no
// accumulate, no activation, 16-B aligned C rows, col_end % 8 == 0.  The output type is
// compile-time; d.bias_kind costs one uniform branch around the bias loads, or nothing
// where the caller passes a constant (the dense kernels).  The rest is straight-line
// code (the generic store_direct of gemm.hip unrolls every runtime combination into ~12k
// instructions).  row0 / col0: the wave's first row / column.
// GLU (bf16 output only): the lane's 8 columns are 4 whole (gate, up) pairs of an interleaved
// gate|up output; their SwiGLU gate, computed from the bf16-rounded values as k_swiglu_fwd_il
// computes it from memory, goes to d.glu[row][col / 2] as one 8-B vector.
template <bool OUT_BF16, bool GLU = false>
__device__ __forceinline__ void store_direct_fast(const TileDst& d, const floatx4 (&acc)[4][4], int row0, int col0,
                                                  int lane) {
  const int c = lane & 15, gq = lane >> 4;
  const int kind = d.bias_kind;
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const int col = col0 + 32 * p + 8 * gq;
    float bias[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) bias[e] = 0.f;
    if (kind == 1 && col < d.col_end) {
#pragma unroll
      for (int e = 0; e < 8; ++e) bias[e] = reinterpret_cast<const float*>(d.bias)[col + e];
    } else if (kind == 2 && col < d.col_end) {
#pragma unroll
      for (int e = 0; e < 8; ++e) bias[e] = bf2f(reinterpret_cast<const uint16_t*>(d.bias)[col + e]);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = row0 + 16 * i + c;
      float v[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = d.alpha * acc[i][2 * p + (e >> 2)][e & 3] + bias[e];
      if (row < d.row_end && col < d.col_end) {
        if constexpr (OUT_BF16) {
          uint32_t w[4];
#pragma unroll
          for (int q = 0; q < 4; ++q) w[q] = pk_bf16(v[2 * q], v[2 * q + 1]);
          *reinterpret_cast<uint4*>(reinterpret_cast<uint16_t*>(d.C) + (size_t)row * d.ldc + col) =
              uint4{w[0], w[1], w[2], w[3]};
          if constexpr (GLU) {
            float a[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
              const float gv = bf16_lo(w[q]);
              a[q] = gv * sigmoid_fast(gv) * bf16_hi(w[q]);
            }
            *reinterpret_cast<uint2*>(reinterpret_cast<uint16_t*>(d.glu) + (size_t)row * d.ldg + (col >> 1)) =
                uint2{pk_bf16(a[0], a[1]), pk_bf16(a[2], a[3])};
          }
        } else {
          float4* C = reinterpret_cast<float4*>(reinterpret_cast<float*>(d.C) + (size_t)row * d.ldc + col);
          C[0] = make_float4(v[0], v[1], v[2], v[3]);
          C[1] = make_float4(v[4], v[5], v[6], v[7]);
        }
      }
    }
  }
}

// Direct epilogue of nn_loop (alpha only): 4 consecutive columns of one row per lane and
// MFMA tile, one 8-B (bf16) or 16-B (fp32) vector store each; col_end % 4 == 0.
template <bool OUT_BF16>
__device__ __forceinline__ void store_direct4(const TileDst& d, const floatx4 (&acc)[4][4], int row0, int col0, int lane) {
  const int c = lane & 15, gq = lane >> 4;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int row = row0 + 16 * i + c;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int col = col0 + 16 * j + 4 * gq;
      if (row < d.row_end && col < d.col_end) {
        const float v0 = d.alpha * acc[i][j][0], v1 = d.alpha * acc[i][j][1], v2 = d.alpha * acc[i][j][2],
                    v3 = d.alpha * acc[i][j][3];
        if constexpr (OUT_BF16)
          *reinterpret_cast<uint2*>(reinterpret_cast<uint16_t*>(d.C) + (size_t)row * d.ldc + col) =
              uint2{pk_bf16(v0, v1), pk_bf16(v2, v3)};
        else
          *reinterpret_cast<float4*>(reinterpret_cast<float*>(d.C) + (size_t)row * d.ldc + col) = make_float4(v0, v1, v2, v3);
      }
    }
  }
}

// Branch-free LDS-staged epilogue of the weight-gradient kernels (fp32 C, alpha only; the
// operand buffers in smem must be dead): lane holds D[4*(lane>>4) + r][lane & 15] of each
// 16x16 tile of the unswapped MFMAs.  ATOMIC = split-K partial sums as lane-consecutive
// fp32 atomics, otherwise plain (or accumulating) 16-B row stores.
template <bool ATOMIC, bool ACCUM>
__device__ __forceinline__ void store_tile_f32(const TileDst& d, floatx4 (&acc)[4][4], unsigned char* smem, int bm,
                                              int bn, int t) {
  const int wave = t >> 6, lane = t & 63;
  const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64;
  float* tile = reinterpret_cast<float*>(smem);
  constexpr int TS = BN + 4;  // fp32 row stride in LDS
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        tile[(wm + i * 16 + (lane >> 4) * 4 + r) * TS + wn + j * 16 + (lane & 15)] = d.alpha * acc[i][j][r];
  __syncthreads();
  float* Cf = reinterpret_cast<float*>(d.C);
  if constexpr (ATOMIC) {
    for (int idx = t; idx < BM * BN; idx += NT) {
      const int rl = idx / BN, cl = idx % BN;
      const int row = bm + rl, col = bn + cl;
      if (row < d.row_end && col < d.col_end) atomicAdd(Cf + (size_t)row * d.ldc + col, tile[rl * TS + cl]);
    }
  } else {
    for (int idx = t; idx < BM * (BN / 4); idx += NT) {
      const int rl = idx / (BN / 4), cl = (idx % (BN / 4)) * 4;
      const int row = bm + rl, col = bn + cl;
      if (row >= d.row_end || col >= d.col_end) continue;
      float4* C = reinterpret_cast<float4*>(Cf + (size_t)row * d.ldc + col);
      float4 v = make_float4(tile[rl * TS + cl], tile[rl * TS + cl + 1], tile[rl * TS + cl + 2], tile[rl * TS + cl + 3]);
      if constexpr (ACCUM) {
        const float4 o = *C;
        v.x += o.x; v.y += o.y; v.z += o.z; v.w += o.w;
      }
      *C = v;
    }
  }
}

}  // namespace gemm
}  // namespace dev
}  // namespace ccmpi
