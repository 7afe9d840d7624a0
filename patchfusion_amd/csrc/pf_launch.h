// Host side of the launchers: the compute-unit count, the dynamic-LDS opt-in and the grid of the persistent GEMMs.  Host code only.
#pragma once
#include <atomic>
#include <limits.h>
#include <stdlib.h>
#include <hip/hip_runtime.h>
#include "pf_common.h"
#include "../../include/pf_hip.h"

// compute units of the current device, asked once per device ordinal (dev & 63); 256 when the query fails (no device)
inline int pf_cu_count() {
  static std::atomic<int> cus[64];
  int dev = 0;
  hipGetDevice(&dev);
  int c = cus[dev & 63].load(std::memory_order_relaxed);
  if (c <= 0) {
    if (hipDeviceGetAttribute(&c, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || c <= 0) c = 256;
    cus[dev & 63].store(c, std::memory_order_relaxed);
  }
  return c;
}

// More than 64 KiB of dynamic LDS is a function attribute that belongs to a DEVICE.  `done` (one static per launcher) keeps one bit per device ordinal
// (dev & 63), set atomically and only after every call succeeded: a second GPU in the same process, or a second host thread, sets the attribute for
// itself, and a failed call is tried again by the next launch.  false: the caller returns PF_ERR_LAUNCH without launching.
template <typename... K>
inline bool pf_ensure_dynamic_lds(std::atomic<unsigned long long>& done, int bytes, K... kernels) {
  int dev = 0;
  hipGetDevice(&dev);
  const unsigned long long bit = 1ull << (dev & 63);
  if (done.load(std::memory_order_acquire) & bit) return true;
  if (!((hipFuncSetAttribute(reinterpret_cast<const void*>(kernels), hipFuncAttributeMaxDynamicSharedMemorySize, bytes) == hipSuccess) && ...)) return false;
  done.fetch_or(bit, std::memory_order_release);
  return true;
}

constexpr int PF_ERR_FALLBACK = -100;     // internal: the persistent launch is not legal for this grid, use the one-tile kernel
constexpr int PF_ERR_REFUSED = -1;        // internal: no legal grid (the launcher returns PF_ERR_ARG)

namespace pf_launch {

// Blocks of a persistent GEMM that walks `total` tiles on a chip of `cus` compute units: one block per CU, a multiple of 8 (8 XCDs on gfx950: the walk
// gives every XCD a contiguous tile range).  `policy` (PF_GRID_*, include/pf_hip.h) says which knobs the launcher honours -- the caller's grid_cap
// (pf_gemm_split3_ex: leave CUs to a concurrent HBM-bound stream), then PF_S3_GRID (tests: fewer blocks than CUs = more tiles per block; read per
// call, overrides the cap; below 8 or not a number = no grid) -- and what fewer than 8 blocks mean: 8 anyway (the blocks of an empty tile range return
// at once), PF_ERR_FALLBACK, or PF_ERR_REFUSED.  More than INT_MAX tiles: PF_ERR_REFUSED.  pf_persist_grid exposes the rule to the CPU tests.
inline int persist_grid(int cus, int grid_cap, long total, int policy) {
  if (total > INT_MAX) return PF_ERR_REFUSED;
  int grid = cus;
  if ((policy & PF_GRID_CAP) && grid_cap > 0 && grid_cap < grid) grid = grid_cap;
  if (policy & PF_GRID_ENV)
    if (const char* s = getenv("PF_S3_GRID")) grid = atoi(s);
  if (grid > total) grid = (int)total;
  grid &= ~7;
  if (grid >= 8) return grid;
  return (policy & PF_GRID_FLOOR8) ? 8 : (policy & PF_GRID_FALLBACK) ? PF_ERR_FALLBACK : PF_ERR_REFUSED;
}

}  // namespace pf_launch
