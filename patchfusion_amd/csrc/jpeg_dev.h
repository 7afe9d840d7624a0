// Device pieces that csrc/jpeg.hip and csrc/jpeg_prog.hip share (as png_dev.h does for the two PNG encoders): the launch helpers and the
// segmented scan that turns DC differences into absolute DCs, one channel per component.  Everything sits in an anonymous namespace, so
// each of the two files gets its own copy of the carry kernel.
#pragma once
#include "pf_common.h"
#include "../../include/pf_hip.h"

namespace {

inline int ok() { return hipGetLastError() == hipSuccess ? PF_OK : PF_ERR_LAUNCH; }
#define ST(s) reinterpret_cast<hipStream_t>(s)

constexpr int JT = 256;                      // threads per block of every kernel here

// ---- segmented scan over DC differences: f = a segment starts here, v0..v2 = the running sums of the three components
struct Dc4 { int f, v0, v1, v2; };
__device__ __forceinline__ Dc4 dc_combine(const Dc4& a, const Dc4& b) {     // a before b
  Dc4 r;
  r.f = a.f | b.f;
  r.v0 = b.f ? b.v0 : a.v0 + b.v0;
  r.v1 = b.f ? b.v1 : a.v1 + b.v1;
  r.v2 = b.f ? b.v2 : a.v2 + b.v2;
  return r;
}
__device__ __forceinline__ Dc4 dc_block_scan(Dc4 x, Dc4* sh) {              // inclusive, over the JT threads of a block
  const int t = threadIdx.x;
  sh[t] = x;
  __syncthreads();
  for (int o = 1; o < JT; o <<= 1) {
    Dc4 y = x;
    if (t >= o) y = dc_combine(sh[t - o], x);
    __syncthreads();
    sh[t] = x = y;
    __syncthreads();
  }
  return x;
}
// exclusive scan of the chunk aggregates, in place (one block; a run of chunks per thread)
__global__ __launch_bounds__(JT) void jpeg_dc_carry_kernel(Dc4* __restrict__ agg, int nchunks) {
  __shared__ Dc4 sh[JT];
  const int t = threadIdx.x, per = (nchunks + JT - 1) / JT;
  const int a = min(t * per, nchunks), e = min(a + per, nchunks);
  Dc4 sum = {0, 0, 0, 0};
  for (int i = a; i < e; ++i) sum = dc_combine(sum, agg[i]);
  dc_block_scan(sum, sh);
  Dc4 run = {0, 0, 0, 0};
  if (t > 0) run = sh[t - 1];
  for (int i = a; i < e; ++i) {
    const Dc4 x = agg[i];
    agg[i] = run;
    run = dc_combine(run, x);
  }
}

}  // namespace
