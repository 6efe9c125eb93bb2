// The per-CTA flag protocol shared by the collective kernels (collectives.hip,
// moe.hip): start barrier with the publication of up to two buffer codes, the
// stage flags, and the epoch write-back.  Device code only; internal linkage, so
// every translation unit gets its own copy.
#pragma once

#include "collectives.hpp"
#include "common.hpp"

namespace ccmpi {
namespace dev {
namespace {

// Per-CTA prologue: bump the epoch, publish up to two buffer codes, barrier.
// Returns false on timeout.  `codes` (LDS) receives every rank's codes.
__device__ bool start_phase(const CollArgs& a, uint64_t* s_epoch, uint64_t (*codes)[kMaxRanks]) {
  const PeerTable* pt = a.pt;
  const int b = blockIdx.x, t = threadIdx.x, me = pt->rank, nr = pt->size;
  if (t == 0) *s_epoch = a.epochs[b] + 1;
  __syncthreads();
  const uint64_t e = *s_epoch;
  Signals* mine = pt->sig[me];
  if (t < nr) {
    Signals* peer = pt->sig[t];
    signal_store(&peer->addr[0][b][me], a.src_code);
    signal_store(&peer->addr[1][b][me], a.res_code);
    // make every prior write of this rank (earlier kernels' output in this
    // XCD's L2, e.g. the tensor we are about to publish) visible system-wide
    release_sys();
    signal_store(&peer->flag[0][b][me], e);
  }
  bool ok = true;
  if (t < nr) {
    ok = wait_geq(&mine->flag[0][b][t], e, a.timeout_ticks, &mine->error, 0x100 + t);
    if (!ok) report_host(pt, 0x100 + t);
    if (ok) {
      codes[0][t] = __hip_atomic_load(&mine->addr[0][b][t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      codes[1][t] = __hip_atomic_load(&mine->addr[1][b][t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
  }
  ok = __syncthreads_and(ok);
  return ok;
}

// Stage flag `phase` (1..3): every thread's stores are drained, then lane j
// tells rank j, then we wait for all ranks.  Returns false on timeout.
__device__ bool sync_phase(const CollArgs& a, int phase, uint64_t e) {
  const PeerTable* pt = a.pt;
  const int b = blockIdx.x, t = threadIdx.x, me = pt->rank, nr = pt->size;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  Signals* mine = pt->sig[me];
  if (t < nr) {
    release_sys();
    signal_store(&pt->sig[t]->flag[phase][b][me], e);
  }
  bool ok = true;
  if (t < nr) {
    ok = wait_geq(&mine->flag[phase][b][t], e, a.timeout_ticks, &mine->error, 0x100 * (phase + 1) + t);
    if (!ok) report_host(pt, 0x100 * (phase + 1) + t);
  }
  ok = __syncthreads_and(ok);
  return ok;
}

__device__ __forceinline__ void finish(const CollArgs& a, uint64_t e) {
  if (threadIdx.x == 0) a.epochs[blockIdx.x] = e;
}

}  // namespace
}  // namespace dev
}  // namespace ccmpi
