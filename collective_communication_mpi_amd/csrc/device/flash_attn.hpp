// Constants of the flash attention kernels (flash_attn.hip).
#pragma once

namespace ccmpi {
namespace dev {

constexpr int kFlashThreads = 256;  // four waves per workgroup, one per SIMD
constexpr int kFlashQT = 2;         // 16-row query tiles per wave (forward and dQ kernels)
// Query rows per workgroup of the forward and the dQ kernel, and keys per step of their key
// loop (= keys per workgroup of the dK/dV kernel).  Together with the fixed loop orders they
// set the summation order of every output: changing them changes last bits, nothing else.
constexpr int kFlashBQ = 4 * 16 * kFlashQT;
constexpr int kFlashBK = 64;
constexpr int kFlashBwdQ = 32;  // query rows per step of the dK/dV kernel

}  // namespace dev
}  // namespace ccmpi
