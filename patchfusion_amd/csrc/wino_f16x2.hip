// fp16x2 form of the three-step Winograd F(4x4,3x3) layer (round 7; host side: csrc/winograd.hip run_f16x2, GEMM: csrc/gemm_split3.hip F16).
//
// The transform-domain GEMM of csrc/winograd.hip run_split3 carries every float32 operand as three bf16 planes and pays six bf16 MFMAs per
// product.  Here each operand is two fp16 planes with a power-of-two scale,  x = 2^e (h + l),  h = fp16_rn(x / 2^e), l = fp16_rn(x / 2^e - h),
// and a product costs three MFMAs (hh, hl, lh; the dropped ll term is <= 2^-22 of |x||w|).  fp16 has 11 significant bits but only five exponent
// bits, so the scale must remove the spread the GEMM sums over -- the K axis (input channels): the RCU / double-conv pairs of the head read channels
// whose magnitudes span six decades, with weights that compensate (tests/dynamic_range.py).  Scale choice, per layer call:
//   m_c = max |relu?(x[..., c])| over every pixel (wino_absmax_kernel: a uint max of non-negative float bits -- order-free, bit-reproducible);
//   e_c = ceil(log2 m_c) + 7 - 15: B^T has absolute row sums <= 10, so |V[p, t, c]| <= 100 m_c < 2^(e_c + 15), inside the fp16 range;
//         m_c = 0 or not finite -> e_c = 0 (a non-finite input then reaches the output as inf / NaN);
//   U'[p, c, n] = U[p, c, n] 2^e_c, and per (point, output column) f_pn = ceil(log2 max_c |U'|) - 15: U' / 2^f_pn is stored as two fp16 planes;
//   M[p, t, n] = ldexp(sum_c V/2^e_c . U'/2^f_pn, f_pn)      -- every scale is a power of two: exact.
// The exponent arithmetic is done on integers (ceil log2 of |U| plus e_c), so no intermediate leaves the float32 range.
#include <climits>
#include "pf_common.h"
#include "../../include/pf_hip.h"
#include "pf_args.h"

namespace {

// ceil(log2 a) for a finite a > 0
__device__ __forceinline__ int clog2(float a) {
  int e;
  const float f = frexpf(a, &e);                        // a = f 2^e, f in [0.5, 1)
  return f == 0.5f ? e - 1 : e;
}
// e_c of a channel from the bits of its absolute maximum
__device__ __forceinline__ int chan_exp(unsigned mb) { return (mb == 0u || mb >= 0x7f800000u) ? 0 : clog2(__uint_as_float(mb)) - 8; }

__device__ __forceinline__ uint32_t pack_h2(_Float16 a, _Float16 b) {
  return (uint32_t)__builtin_bit_cast(uint16_t, a) | ((uint32_t)__builtin_bit_cast(uint16_t, b) << 16);
}

// m_c = max over P pixels of |relu?(x[r][c])| as float bits: thread (c4, r0) walks pixels r0, r0 + R, ... of channel quad c4, keeps its maximum in
// registers, merges it into the block's LDS copy, and the block merges that into cmax (uint atomics: the order does not matter, the result is exact).
__global__ __launch_bounds__(256) void wino_absmax_kernel(const float* __restrict__ x, int x_ld, long P, int C, int relu_in, long R,
                                                          unsigned* __restrict__ cmax) {
  extern __shared__ unsigned sm[];
  const int cv = C >> 2;
  for (int i = threadIdx.x; i < C; i += blockDim.x) sm[i] = 0u;
  __syncthreads();
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx < (long)cv * R) {
    const int c4 = (int)(idx % cv);
    long r = idx / cv;
    const float* xp = x + c4 * 4;
    uint32_t m[4] = {0u, 0u, 0u, 0u};
    auto take = [&](float4 v) __attribute__((always_inline)) {
      if (relu_in) { v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f); }
      m[0] = max(m[0], __float_as_uint(v.x) & 0x7fffffffu);
      m[1] = max(m[1], __float_as_uint(v.y) & 0x7fffffffu);
      m[2] = max(m[2], __float_as_uint(v.z) & 0x7fffffffu);
      m[3] = max(m[3], __float_as_uint(v.w) & 0x7fffffffu);
    };
    for (; r + 3 * R < P; r += 4 * R) {                 // four independent loads in flight per thread
      const float4 a = *reinterpret_cast<const float4*>(xp + r * x_ld);
      const float4 b = *reinterpret_cast<const float4*>(xp + (r + R) * x_ld);
      const float4 c = *reinterpret_cast<const float4*>(xp + (r + 2 * R) * x_ld);
      const float4 d = *reinterpret_cast<const float4*>(xp + (r + 3 * R) * x_ld);
      take(a); take(b); take(c); take(d);
    }
    for (; r < P; r += R) take(*reinterpret_cast<const float4*>(xp + r * x_ld));
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (m[e]) atomicMax(&sm[c4 * 4 + e], m[e]);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < C; i += blockDim.x)
    if (sm[i]) atomicMax(&cmax[i], sm[i]);
}

// U' planes: one wave per (transform point, filter row n).  f = max_c (ceil log2 |U| + e_c) - 15 over the finite non-zero entries (0 for a zero row),
// U'/2^f = ldexp(U, e_c - f) split into h / l, written chunk-major [2][36][C/32][rows][32] fp16; fexp[pt][n] = f.
__global__ __launch_bounds__(256) void wino_u_split_kernel(const float* __restrict__ U, int rows, int C, int npts, const unsigned* __restrict__ cmax,
                                                           uint16_t* __restrict__ U2, int* __restrict__ fexp) {
  const int wv = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (wv >= npts * rows) return;
  const int pt = wv / rows, n = wv - pt * rows;
  const float* u = U + ((long)pt * rows + n) * C;
  int mx = INT_MIN;
  for (int c = lane; c < C; c += 64) {
    const float a = fabsf(u[c]);
    if (a != 0.f && a < INFINITY) mx = max(mx, clog2(a) + chan_exp(cmax[c]));
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) mx = max(mx, __shfl_xor(mx, o));
  const int f = mx == INT_MIN ? 0 : mx - 15;
  const size_t plane = (size_t)npts * C * rows;
  for (int c = lane; c < C; c += 64) {
    const float v = ldexpf(u[c], chan_exp(cmax[c]) - f);
    const _Float16 h = (_Float16)v, l = (_Float16)(v - (float)h);
    const size_t o = (((size_t)pt * (C >> 5) + (c >> 5)) * rows + n) * 32 + (c & 31);
    U2[o] = __builtin_bit_cast(uint16_t, h);
    U2[o + plane] = __builtin_bit_cast(uint16_t, l);
  }
  if (lane == 0) fexp[pt * rows + n] = f;
}

// B^T d B of F(4x4,3x3) along one axis (the same arithmetic as csrc/winograd.hip Wino<4>::bt)
__device__ __forceinline__ void bt6(float (&d)[6]) {
  const float o0 = 4.f * d[0] - 5.f * d[2] + d[4];
  const float o1 = -4.f * (d[1] + d[2]) + d[3] + d[4];
  const float o2 = 4.f * (d[1] - d[2]) - d[3] + d[4];
  const float o3 = -2.f * d[1] - d[2] + 2.f * d[3] + d[4];
  const float o4 = 2.f * d[1] - d[2] - 2.f * d[3] + d[4];
  const float o5 = 4.f * d[1] - 5.f * d[3] + d[5];
  d[0] = o0; d[1] = o1; d[2] = o2; d[3] = o3; d[4] = o4; d[5] = o5;
}

// input transform of one tile window into V / 2^e_c as two fp16 planes, chunk-major [2][36][C/32][T][32]: the thread order and the tile octets of
// csrc/winograd.hip wino_input_kernel<4, true> (8 lanes = the 8 channel quads of one 32-channel chunk of one tile), 8 + 8 bytes stored per point
__global__ __launch_bounds__(512) void wino_input_f16x2_kernel(const float* __restrict__ x, int x_ld, int B, int H, int W, int C, int relu_in,
                                                               const unsigned* __restrict__ cmax, uint16_t* __restrict__ V, int TH, int TW, long total,
                                                               long tile0, long T) {
  constexpr int MT = 4, A = 6;
  const int nkc = C >> 5;
  for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
    const long w64 = idx >> 6;
    const long tile = (w64 / nkc) * 8 + ((idx >> 3) & 7);
    const int c4 = (int)(w64 % nkc) * 8 + (int)(idx & 7);
    if (tile >= T) continue;
    const long gt = tile + tile0;
    const int tx = (int)(gt % TW), ty = (int)((gt / TW) % TH), b = (int)(gt / ((long)TW * TH));
    const uint4 mb = *reinterpret_cast<const uint4*>(cmax + c4 * 4);
    const int ne[4] = {-chan_exp(mb.x), -chan_exp(mb.y), -chan_exp(mb.z), -chan_exp(mb.w)};
    float d[A][A][4];
#pragma unroll
    for (int i = 0; i < A; ++i) {
      const int y = ty * MT - 1 + i;
#pragma unroll
      for (int j = 0; j < A; ++j) {
        const int xx = tx * MT - 1 + j;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if ((unsigned)y < (unsigned)H && (unsigned)xx < (unsigned)W)
          v = *reinterpret_cast<const float4*>(x + (((long)b * H + y) * W + xx) * x_ld + c4 * 4);
        if (relu_in) { v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f); }
        d[i][j][0] = v.x; d[i][j][1] = v.y; d[i][j][2] = v.z; d[i][j][3] = v.w;
      }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
#pragma unroll
      for (int j = 0; j < A; ++j) {
        float col[A];
#pragma unroll
        for (int i = 0; i < A; ++i) col[i] = d[i][j][e];
        bt6(col);
#pragma unroll
        for (int i = 0; i < A; ++i) d[i][j][e] = col[i];
      }
#pragma unroll
      for (int i = 0; i < A; ++i) {
        float row[A];
#pragma unroll
        for (int j = 0; j < A; ++j) row[j] = d[i][j][e];
        bt6(row);
#pragma unroll
        for (int j = 0; j < A; ++j) d[i][j][e] = row[j];
      }
    }
    const size_t plane = (size_t)T * C;
    uint16_t* o = V + ((size_t)(c4 >> 3) * T + tile) * 32 + (c4 & 7) * 4;
#pragma unroll
    for (int i = 0; i < A; ++i)
#pragma unroll
      for (int j = 0; j < A; ++j) {
        _Float16 h[4], l[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float v = ldexpf(d[i][j][e], ne[e]);
          h[e] = (_Float16)v;
          l[e] = (_Float16)(v - (float)h[e]);
        }
        uint16_t* q = o + (size_t)(i * A + j) * plane;
        *reinterpret_cast<uint2*>(q) = make_uint2(pack_h2(h[0], h[1]), pack_h2(h[2], h[3]));
        *reinterpret_cast<uint2*>(q + (size_t)A * A * plane) = make_uint2(pack_h2(l[0], l[1]), pack_h2(l[2], l[3]));
      }
  }
}

}  // namespace

// launch helpers for csrc/winograd.hip run_f16x2 (not part of the C ABI)
namespace pf_f16x2 {

int launch_absmax(const float* x, int x_ld, long P, int C, int relu_in, unsigned* cmax, hipStream_t st) {
  const int cv = C >> 2;
  long R = (256L * 2048L) / cv;                         // ~2k threads per CU of a 256-CU chip; each walks pixels R apart
  if (R < 1) R = 1;
  if (R > P) R = P;
  const long threads = (long)cv * R;
  hipLaunchKernelGGL(wino_absmax_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), (size_t)C * 4, st, x, x_ld, P, C, relu_in, R, cmax);
  return hipGetLastError() == hipSuccess ? PF_OK : PF_ERR_LAUNCH;
}

int launch_u_split(const float* U, int rows, int C, const unsigned* cmax, void* U2, int* fexp, hipStream_t st) {
  const long waves = 36L * rows;
  hipLaunchKernelGGL(wino_u_split_kernel, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, st, U, rows, C, 36, cmax, static_cast<uint16_t*>(U2), fexp);
  return hipGetLastError() == hipSuccess ? PF_OK : PF_ERR_LAUNCH;
}

int launch_input(const float* x, int x_ld, int B, int H, int W, int C, int relu_in, const unsigned* cmax, void* V, int TH, int TW, long tile0, long T,
                 hipStream_t st) {
  const long nin = ((T + 7) / 8) * 8 * (C / 4);
  hipLaunchKernelGGL(wino_input_f16x2_kernel, dim3((unsigned)((nin + 255) / 256)), dim3(256), 0, st, x, x_ld, B, H, W, C, relu_in, cmax,
                     static_cast<uint16_t*>(V), TH, TW, nin, tile0, T);
  return hipGetLastError() == hipSuccess ? PF_OK : PF_ERR_LAUNCH;
}

}  // namespace pf_f16x2
