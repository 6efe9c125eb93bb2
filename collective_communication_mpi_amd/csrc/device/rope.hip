// Rotary position embedding (ops.rope_apply, ops.rope): q [B, S, Hq, D] and, optionally,
// k [B, S, Hkv, D] (packed: [T, Hq, D] / [T, Hkv, D]) rotated in ONE launch.  bf16 in and out, fp32
// arithmetic, one rounding to bf16 per element.  Operands and outputs are views under the rules of
// flash attention (unit stride on D, every other stride a multiple of 8 elements, 16-byte-aligned
// base), each with strides of its own; an output may BE its input: every element is read and
// written by the same thread, and a thread reads all it owns of a group of heads before it writes
// any of it.  All address arithmetic is 64-bit; no atomics; D is a runtime value, D % 16 == 0.
//
//   table    [P, 2, D / 2] fp32, contiguous: table[p, 0, j] = cos(p f_j), table[p, 1, j] = sin(p f_j).
//            The kernel calls no trigonometric function; the angles are the caller's.
//   pairing  half-split (x[j], x[j + D/2]) or, INTERLEAVED, (x[2j], x[2j + 1]); frequency index j
//            in both.  Both go through rotate(): y1 = x1 c - x2 s, y2 = x2 c + x1 s, each one
//            rounded product and one FMA, spelled with intrinsics so that no instantiation
//            contracts differently from another.  inverse: s -> -s (the transpose = the backward).
//   position PACKED = false: pos0 + s for sequence index s (pos0 >= 0 a host scalar).
//            PACKED = true: t - begin for token t of the sequence that owns it, begin = clamp(cu[i],
//            0, T), end = clamp(cu[i + 1], begin, T), found by bisection over cu ON THE DEVICE, once
//            per token: thread i of a workgroup bisects for the workgroup's i-th token and hands
//            the position round through LDS.  Tokens outside every sequence (before cu[0], from
//            cu[n] on) are neither read nor written.
//            Both: the table row is min(position, P - 1), so no content of cu makes an address
//            leave a tensor.
//
// Mapping: a thread owns one 8-pair slice of D of one token -- two 16-byte runs of x, two 32-byte
// runs of the table row, loaded once -- and walks the concatenated head axis (q's heads, then k's)
// with them in steps of `lanes` heads, kRopeInFlight heads' loads issued before the first store.
// A token's threads are (head lane, slice), lanes = rope_head_lanes(slices, heads, packed): one
// wave-wide load covers contiguous runs of ONE token (8 heads x 128 bytes, 256 bytes apart, at
// D = 128; the second load fills the gaps), which measured 15-25 % faster at the Llama-3-8B shape
// than giving each lane a token of its own and all of that token's heads.  The table slice is so
// read once per head lane of a token (from cache), not once per token, and a token whose threads
// straddle two workgroups is bisected in both.  The grid depends on T, the heads and D alone.
#include <hip/hip_runtime.h>
#include <pybind11/pybind11.h>

#include <climits>
#include <stdexcept>
#include <string>
#include <tuple>

#include "common.hpp"
#include "ops.hpp"
#include "rope.hpp"

namespace ccmpi {
namespace dev {

namespace {

constexpr int kThreads = kRopeThreads;

// One operand with its output: element strides of the batch, token and head axes.
struct RopeSide {
  const uint16_t* in;
  uint16_t* out;
  int64_t ib, it, ih, ob, ot, oh;
  int H;
};

struct RopeArgs {
  RopeSide q, k;       // k.H = 0: no k
  const float* table;  // [P, 2, D / 2]
  const int* cu;       // PACKED: n + 1 boundaries
  int64_t N, S;        // tokens in all (B S, or T) and per batch entry
  int64_t pos0;
  int n, P, D, slices, lanes;
  int inverse;
};

// The one place the arithmetic lives: a rounded product, then one FMA, for each output.
__device__ __forceinline__ void rotate(float x1, float x2, float c, float s, float& y1, float& y2) {
  y1 = __fmaf_rn(x1, c, -__fmul_rn(x2, s));
  y2 = __fmaf_rn(x2, c, __fmul_rn(x1, s));
}

// a, b: the thread's two 16-byte runs of one head.  Half-split: a = x1[0..8), b = x2[0..8).
// Interleaved: a = pairs 0..3, b = pairs 4..7, x1 the low and x2 the high half of each word.
template <bool INTERLEAVED>
__device__ __forceinline__ void rotate8(u32x4& a, u32x4& b, const float (&c)[8], const float (&s)[8]) {
  float y1[8], y2[8];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (INTERLEAVED) {
      rotate(bf16_lo(a[i]), bf16_hi(a[i]), c[i], s[i], y1[i], y2[i]);
      rotate(bf16_lo(b[i]), bf16_hi(b[i]), c[4 + i], s[4 + i], y1[4 + i], y2[4 + i]);
    } else {
      rotate(bf16_lo(a[i]), bf16_lo(b[i]), c[2 * i], s[2 * i], y1[2 * i], y2[2 * i]);
      rotate(bf16_hi(a[i]), bf16_hi(b[i]), c[2 * i + 1], s[2 * i + 1], y1[2 * i + 1], y2[2 * i + 1]);
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (INTERLEAVED) {
      a[i] = pk_bf16(y1[i], y2[i]);
      b[i] = pk_bf16(y1[4 + i], y2[4 + i]);
    } else {
      a[i] = pk_bf16(y1[2 * i], y1[2 * i + 1]);
      b[i] = pk_bf16(y2[2 * i], y2[2 * i + 1]);
    }
  }
}

// PACKED: position of token t inside its sequence, -1 when no sequence owns it.  The sequence is
// the last one that starts at or before t (empty ones before it start there too and end there).
__device__ __forceinline__ int packed_position(const int* cu, int n, int T, int t) {
  auto at = [&](int i) { return min(max(cu[i], 0), T); };
  if (at(0) > t) return -1;
  int lo = 0, hi = n;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (at(mid) <= t) lo = mid; else hi = mid;
  }
  const int begin = at(lo), end = max(at(lo + 1), begin);
  return t < end ? t - begin : -1;
}

template <bool PACKED, bool INTERLEAVED>
__global__ void __launch_bounds__(kThreads) k_rope(const RopeArgs p) {
  const int lanes = p.lanes, per_tok = p.slices * lanes;  // threads of one token: (head lane, slice)
  const int64_t gid = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  const int64_t tok = gid / per_tok;
  const int rem = (int)(gid - tok * per_tok);
  const int hl = rem / p.slices, slice = rem - hl * p.slices;
  int64_t pos;
  if (PACKED) {
    __shared__ int s_pos[kThreads];
    const int64_t first = (int64_t)blockIdx.x * kThreads / per_tok;  // this workgroup's first token
    const int64_t mine = first + threadIdx.x;
    const int64_t last = ((int64_t)blockIdx.x * kThreads + kThreads - 1) / per_tok;
    if (mine <= last && mine < p.N) s_pos[threadIdx.x] = packed_position(p.cu, p.n, (int)p.N, (int)mine);
    __syncthreads();
    if (tok >= p.N) return;
    pos = s_pos[tok - first];
    if (pos < 0) return;
  } else {
    if (tok >= p.N) return;
    pos = p.pos0 + tok % p.S;
  }
  const int64_t row = pos < p.P ? pos : p.P - 1;
  const float* tc = p.table + row * p.D + 8 * slice;
  const float4 c0 = *reinterpret_cast<const float4*>(tc), c1 = *reinterpret_cast<const float4*>(tc + 4);
  const float4 s0 = *reinterpret_cast<const float4*>(tc + p.D / 2), s1 = *reinterpret_cast<const float4*>(tc + p.D / 2 + 4);
  const float c[8] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w};
  float s[8] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w};
  if (p.inverse) {
#pragma unroll
    for (int i = 0; i < 8; ++i) s[i] = -s[i];
  }
  const int64_t b = PACKED ? 0 : tok / p.S, t = PACKED ? tok : tok - b * p.S;
  const int first_el = INTERLEAVED ? 16 * slice : 8 * slice;
  const int second = INTERLEAVED ? 8 : p.D / 2;
  const uint16_t* qi = p.q.in + b * p.q.ib + t * p.q.it + first_el;
  uint16_t* qo = p.q.out + b * p.q.ob + t * p.q.ot + first_el;
  const uint16_t* ki = p.k.in + b * p.k.ib + t * p.k.it + first_el;
  uint16_t* ko = p.k.out + b * p.k.ob + t * p.k.ot + first_el;
  // heads hl, hl + lanes, ... of the concatenated axis [q's heads | k's heads]; no __restrict__:
  // an output may be its input, so a group's loads all come before its first store
  const int Hq = p.q.H, H = p.q.H + p.k.H;
  for (int g = hl; g < H; g += lanes * kRopeInFlight) {
    u32x4 a[kRopeInFlight], bb[kRopeInFlight];
#pragma unroll
    for (int i = 0; i < kRopeInFlight; ++i) {
      const int gi = g + i * lanes;
      if (gi < H) {
        const uint16_t* src = gi < Hq ? qi + (int64_t)gi * p.q.ih : ki + (int64_t)(gi - Hq) * p.k.ih;
        a[i] = *reinterpret_cast<const u32x4*>(src);
        bb[i] = *reinterpret_cast<const u32x4*>(src + second);
      }
    }
#pragma unroll
    for (int i = 0; i < kRopeInFlight; ++i) {
      const int gi = g + i * lanes;
      if (gi < H) {
        rotate8<INTERLEAVED>(a[i], bb[i], c, s);
        uint16_t* dst = gi < Hq ? qo + (int64_t)gi * p.q.oh : ko + (int64_t)(gi - Hq) * p.k.oh;
        *reinterpret_cast<u32x4*>(dst) = a[i];
        *reinterpret_cast<u32x4*>(dst + second) = bb[i];
      }
    }
  }
}

[[noreturn]] void refuse(const std::string& what) { throw std::invalid_argument("rope: " + what); }

// (address, batch stride, token stride, head stride) in elements; 0 for an axis of length 1
using View = std::tuple<uint64_t, int64_t, int64_t, int64_t>;

void check_view(const char* what, const View& v) {
  const auto [ptr, b, t, h] = v;
  if (ptr == 0 || ptr % 16) refuse(std::string(what) + " must be 16-byte aligned");
  if (b % 8 || t % 8 || h % 8) refuse(std::string(what) + " strides must be multiples of 8 elements");
}

RopeSide side(const View& in, const View& out, int64_t H) {
  return {reinterpret_cast<const uint16_t*>(std::get<0>(in)), reinterpret_cast<uint16_t*>(std::get<0>(out)),
          std::get<1>(in), std::get<2>(in), std::get<3>(in), std::get<1>(out), std::get<2>(out), std::get<3>(out), (int)H};
}

void rope_apply(View q, View q_out, int64_t Hq, View k, View k_out, int64_t Hkv, uint64_t table, int64_t P, int64_t B,
                int64_t S, int64_t D, int64_t pos0, uint64_t cu_seqlens, int64_t n_seq, bool interleaved, bool inverse,
                int64_t lanes, uint64_t stream) {
  if (D < 16 || D > 256 || D % 16) refuse("the head dim must be a multiple of 16 in [16, 256]");
  if (Hq < 1 || Hq > 65535 || Hkv < 0 || Hkv > 65535) refuse("1 <= Hq <= 65535 and 0 <= Hkv <= 65535 required");
  if (B < 1 || S < 1 || B > (1 << 30) / S) refuse("1 <= B S <= 2^30 tokens required");
  if (P < 1 || P > (1 << 30)) refuse("1 <= P <= 2^30 table rows required");
  if (table == 0 || table % 16) refuse("the table must be 16-byte aligned");
  if (!cu_seqlens && n_seq) refuse("sequences without cu_seqlens");
  if (cu_seqlens) {
    if (cu_seqlens % 4) refuse("cu_seqlens must be 4-byte aligned");
    if (n_seq < 1 || n_seq > kRopeMaxSeqs) refuse("1 <= n <= 65536 sequences required");
    if (B != 1 || pos0 != 0) refuse("the packed form needs B = 1 and pos0 = 0");
  } else if (pos0 < 0 || pos0 + S > P) {
    refuse("0 <= pos0 and pos0 + S <= P required");
  }
  check_view("q", q);
  check_view("q_out", q_out);
  if (Hkv) {
    check_view("k", k);
    check_view("k_out", k_out);
  }
  const int64_t N = B * S, slices = D / 16, H = Hq + Hkv;
  if (lanes == 0) lanes = rope_head_lanes(slices, H, cu_seqlens != 0);
  if (lanes < 1 || lanes > H) refuse("1 <= lanes <= Hq + Hkv required");
  const int64_t blocks = (N * slices * lanes + kThreads - 1) / kThreads;
  if (blocks > INT_MAX) refuse("tokens x D / 16 x head lanes must stay below 2^39 (the grid)");
  RopeArgs a{side(q, q_out, Hq), Hkv ? side(k, k_out, Hkv) : RopeSide{nullptr, nullptr, 0, 0, 0, 0, 0, 0, 0},
             reinterpret_cast<const float*>(table), reinterpret_cast<const int*>(cu_seqlens), N, S, pos0, (int)n_seq,
             (int)P, (int)D, (int)slices, (int)lanes, inverse ? 1 : 0};
  const dim3 grid((unsigned)blocks);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (cu_seqlens) {
    if (interleaved) hipLaunchKernelGGL((k_rope<true, true>), grid, dim3(kThreads), 0, st, a);
    else hipLaunchKernelGGL((k_rope<true, false>), grid, dim3(kThreads), 0, st, a);
  } else {
    if (interleaved) hipLaunchKernelGGL((k_rope<false, true>), grid, dim3(kThreads), 0, st, a);
    else hipLaunchKernelGGL((k_rope<false, false>), grid, dim3(kThreads), 0, st, a);
  }
  CCMPI_HIP_CHECK(hipGetLastError());
}

}  // namespace

void register_rope_ops(pybind11::module_& m) {
  namespace py = pybind11;
  m.attr("ROPE_MAX_SEQS") = kRopeMaxSeqs;
  m.def("rope_head_lanes", [](int64_t slices, int64_t H, bool packed) { return rope_head_lanes(slices, H, packed); },
        py::arg("slices"), py::arg("H"), py::arg("packed"));
  m.def("rope_apply", &rope_apply,
        "rotate q [B, S, Hq, D] and (Hkv > 0) k [B, S, Hkv, D] bf16 into q_out / k_out (an output may be its input): "
        "views are (address, batch, token, head stride) in elements; table [P, 2, D / 2] fp32 of cos | sin; position "
        "pos0 + s, or with cu_seqlens (device address of n_seq + 1 int32 boundaries, B = 1) the token's index inside "
        "its sequence, read on the device; table row clamped to P - 1.  lanes = 0: rope_head_lanes(D / 16, Hq + Hkv, packed)",
        py::arg("q"), py::arg("q_out"), py::arg("Hq"), py::arg("k"), py::arg("k_out"), py::arg("Hkv"), py::arg("table"),
        py::arg("P"), py::arg("B"), py::arg("S"), py::arg("D"), py::arg("pos0"), py::arg("cu_seqlens"),
        py::arg("n_seq"), py::arg("interleaved"), py::arg("inverse"), py::arg("lanes"), py::arg("stream"),
        py::call_guard<py::gil_scoped_release>());
}

}  // namespace dev
}  // namespace ccmpi
