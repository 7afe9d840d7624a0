// Winograd F(m x m, 3 x 3) path of the float32 ("exact") mode for the large 3x3 / stride-1 / pad-1 convolutions of the DPT head and
// the guided-fusion U-Net (estimator/models/blocks/guided_fusion_model.py:41-48,85-100; external/depth_anything/dpt.py, blocks.py
// ResidualConvUnit) -- 77 % of the f32 image pass is spent in those layers (profiles/r2b_op_roofline_fp32.md).
//
//   Y = A^T [ sum_c (G g G^T) .* (B^T d B) ] A          (Lavin & Gray; m = 2: 2.25x, m = 4: 4x fewer multiplies than direct)
//
// Three steps per layer, the middle one on the matrix cores through the existing f32 implicit-GEMM kernel:
//   1. wino_input_kernel   x NHWC [B,H,W,C]           -> V [(m+2)^2][T][C]      T = B * ceil(H/m) * ceil(W/m) tiles  (HBM-bound)
//   2. pf_conv (1x1)       V[k] [T][C] x U[k] [N][C]  -> M[k] [T][N]           (m+2)^2 GEMM planes in ONE batched launch, U = G g G^T
//   3. wino_output_kernel  M [(m+2)^2][T][N]          -> y NHWC [B,H,W,N]  + bias, ReLU, residual(s)                 (HBM-bound)
// The transforms are exact small-integer / dyadic combinations evaluated in float32; the result differs from the direct
// convolution only by rounding (measured per layer: m = 2 ~2.5x, m = 4 ~15x the rounding error of a direct f32 convolution,
// DESIGN.md 4d).  Only float32 tensors; everything else stays on the direct kernels.
#include <mutex>
#include "pf_common.h"
#include "../../include/pf_hip.h"
#include "pf_args.h"
#include "pf_launch.h"

// csrc/wino_f16x2.hip
namespace pf_f16x2 {
int launch_absmax(const float* x, int x_ld, long P, int C, int relu_in, unsigned* cmax, hipStream_t st);
int launch_u_split(const float* U, int rows, int C, const unsigned* cmax, void* U2, int* fexp, hipStream_t st);
int launch_input(const float* x, int x_ld, int B, int H, int W, int C, int relu_in, const unsigned* cmax, void* V, int TH, int TW, long tile0, long T,
                 hipStream_t st);
int launch_output_cmax(const float* M, const pf_conv_params* p, int TH, int TW, long t0, long T, unsigned* cmax, int cmax_relu, hipStream_t st);
}  // namespace pf_f16x2

namespace {

#define ST(s) reinterpret_cast<hipStream_t>(s)

template <int MT> struct Wino;
template <> struct Wino<2> {
  // B^T = [1 0 -1 0; 0 1 1 0; 0 -1 1 0; 0 1 0 -1]      A^T = [1 1 1 0; 0 1 -1 -1]
  __device__ static __forceinline__ void bt(float (&d)[4]) {
    const float o0 = d[0] - d[2], o1 = d[1] + d[2], o2 = d[2] - d[1], o3 = d[1] - d[3];
    d[0] = o0; d[1] = o1; d[2] = o2; d[3] = o3;
  }
  __device__ static __forceinline__ void at(const float (&m)[4], float (&o)[2]) {
    o[0] = m[0] + m[1] + m[2];
    o[1] = m[1] - m[2] - m[3];
  }
};
template <> struct Wino<4> {
  // B^T = [4 0 -5 0 1 0; 0 -4 -4 1 1 0; 0 4 -4 -1 1 0; 0 -2 -1 2 1 0; 0 2 -1 -2 1 0; 0 4 0 -5 0 1]
  // A^T = [1 1 1 1 1 0; 0 1 -1 2 -2 0; 0 1 1 4 4 0; 0 1 -1 8 -8 1]
  __device__ static __forceinline__ void bt(float (&d)[6]) {
    const float o0 = 4.f * d[0] - 5.f * d[2] + d[4];
    const float o1 = -4.f * (d[1] + d[2]) + d[3] + d[4];
    const float o2 = 4.f * (d[1] - d[2]) - d[3] + d[4];
    const float o3 = -2.f * d[1] - d[2] + 2.f * d[3] + d[4];
    const float o4 = 2.f * d[1] - d[2] - 2.f * d[3] + d[4];
    const float o5 = 4.f * d[1] - 5.f * d[3] + d[5];
    d[0] = o0; d[1] = o1; d[2] = o2; d[3] = o3; d[4] = o4; d[5] = o5;
  }
  __device__ static __forceinline__ void at(const float (&m)[6], float (&o)[4]) {
    const float s12 = m[1] + m[2], d12 = m[1] - m[2], s34 = m[3] + m[4], d34 = m[3] - m[4];
    o[0] = m[0] + s12 + s34;
    o[1] = d12 + 2.f * d34;
    o[2] = s12 + 4.f * s34;
    o[3] = d12 + 8.f * d34 + m[5];
  }
};

// one thread = one tile x 4 channels: (m+2)^2 16-byte loads (zero outside the image = the conv's padding), B^T d B in registers,
// (m+2)^2 16-byte stores into the planes of V.  Consecutive lanes take consecutive channel groups: every load / store of a wave is
// a contiguous 1 KiB run of one pixel / one V row.
// SPLIT: V is written as the three bf16 planes of the split-precision GEMM (csrc/gemm_split3.hip), CHUNK-MAJOR: [3][(m+2)^2][C/32][T][32] bf16
// (every 32-channel K chunk of all tiles is one slab = what the GEMM's 1-KiB DMA pieces read as whole cache lines).  Thread order for that
// layout: 8 lanes = the 8 channel quads of one chunk of one tile (64 B of a slab row, 128 B of a pixel), 8 tiles per wave -> every store
// of a wave is one contiguous 512-byte run of a slab; then the chunks of the same 8 tiles.
// Grid-stride: a launch with fewer blocks than work items walks them (`total` items, blockDim.x at a time) -- the RESIDENT form (512 threads per
// block = one block per CU at these register counts, grid = the number of CUs the transform may take) that runs beside a capped persistent GEMM of
// the other tile batch (run_split3); a launch with one block per 256 items is the plain one-shot form.
// (Measured and NOT kept, round 5: the plane stores as 16-byte stores -- lane pairs trading halves through DPP quad_perm so that every store instruction
// writes a full KiB: three instructions per two transform points instead of six.  Image pass 193.0 vs 193.2 ms, the kernel's own total +3 %
// (profiles/r5_image_ab_pair.md): at full-chip occupancy the input transform is bound by HBM, not by store issue.  Confined to 64 CUs the same kernel runs
// 3x slower -- ~16 B/clk/CU of store issue -- which is why the transforms cannot hide on a CU subset beside the GEMM, profiles/r5_overlap_probe_resident.md.)
template <int MT, bool SPLIT = false>
__global__ __launch_bounds__(512) void wino_input_kernel(const float* __restrict__ x, int x_ld, int B, int H, int W, int C, int relu_in,
                                                         float* __restrict__ V, int TH, int TW, long total, long tile0, long T) {
  // (tile window, round 5: this launch transforms tiles [tile0, tile0 + T) of the layer's B * TH * TW tiles into a V of T rows -- run_split3 walks a
  // layer in windows small enough for the arena pair to stay in the 256 MB memory-side cache)
  constexpr int A = MT + 2;
  const int cv = C >> 2;
  for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
  int c4;
  long tile;
  if constexpr (SPLIT) {
    const int nkc = C >> 5;                           // C % 32 == 0
    const long w64 = idx >> 6;                        // (tile octet, chunk) pairs, chunk fastest
    tile = (w64 / nkc) * 8 + ((idx >> 3) & 7);
    c4 = (int)(w64 % nkc) * 8 + (int)(idx & 7);
    if (tile >= T) continue;
  } else {
    if (idx >= T * cv) continue;
    c4 = (int)(idx % cv);
    tile = idx / cv;
  }
  const long gt = tile + tile0;                       // position of the tile in the layer
  const int tx = (int)(gt % TW), ty = (int)((gt / TW) % TH), b = (int)(gt / ((long)TW * TH));
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
    for (int j = 0; j < A; ++j) {                     // B^T d : along the rows
      float col[A];
#pragma unroll
      for (int i = 0; i < A; ++i) col[i] = d[i][j][e];
      Wino<MT>::bt(col);
#pragma unroll
      for (int i = 0; i < A; ++i) d[i][j][e] = col[i];
    }
#pragma unroll
    for (int i = 0; i < A; ++i) {                     // (B^T d) B : along the columns
      float row[A];
#pragma unroll
      for (int j = 0; j < A; ++j) row[j] = d[i][j][e];
      Wino<MT>::bt(row);
#pragma unroll
      for (int j = 0; j < A; ++j) d[i][j][e] = row[j];
    }
  }
  const size_t plane = (size_t)T * C;
  if constexpr (SPLIT) {
    bf16_t* o = reinterpret_cast<bf16_t*>(V) + ((size_t)(c4 >> 3) * T + tile) * 32 + (c4 & 7) * 4;
#pragma unroll
    for (int i = 0; i < A; ++i)
#pragma unroll
      for (int j = 0; j < A; ++j) store_split3(o + (size_t)(i * A + j) * plane, (long)(A * A) * (long)plane, d[i][j]);
  } else {
    float* o = V + (size_t)tile * C + c4 * 4;
#pragma unroll
    for (int i = 0; i < A; ++i)
#pragma unroll
      for (int j = 0; j < A; ++j)
        *reinterpret_cast<float4*>(o + (size_t)(i * A + j) * plane) = make_float4(d[i][j][0], d[i][j][1], d[i][j][2], d[i][j][3]);
  }
  }
}

// one thread = one tile x 4 output channels: (m+2)^2 16-byte loads from the planes of M, A^T m A, then the conv epilogue in the order of
// pf_conv (bias -> act -> + res -> + res2) and m x m 16-byte stores (bounds-checked: H, W need not be multiples of m)
// (The residual steps are written out, and wino_output_cmax_kernel of csrc/wino_f16x2_n256.hip repeats this body, on purpose.  Tried and not kept,
// each for a different scalar preamble around the same arithmetic: the whole body, grid-stride loop included, in a __device__ __forceinline__ template --
// blockDim.x is then no longer folded from __launch_bounds__(512) but loaded from the dispatch packet, and scalar allocation shifts from there; the loop
// kept here and only the per-item body shared, or only csrc/pf_epilogue.h's epi_add_res for the residuals -- the helper's pointer parameters are generic,
// the null tests of bias / res / res2 compare against a cast null, and the loop-invariant plane offsets are hoisted in another order.)
template <int MT>
__global__ __launch_bounds__(512) void wino_output_kernel(const float* __restrict__ M, int N, const float* __restrict__ bias, int relu,
                                                          const float* __restrict__ res, int res_ld, const float* __restrict__ res2,
                                                          int res2_ld, float* __restrict__ y, int y_ld, int B, int H, int W, int TH,
                                                          int TW, long tile0, long T) {
  constexpr int A = MT + 2;
  const int nv = N >> 2;
  for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < T * nv; idx += (long)gridDim.x * blockDim.x) {      // (grid-stride: see wino_input_kernel)
  const int n4 = (int)(idx % nv);
  const long tile = idx / nv;
  const long gt = tile + tile0;
  const int tx = (int)(gt % TW), ty = (int)((gt / TW) % TH), b = (int)(gt / ((long)TW * TH));
  const size_t plane = (size_t)T * N;
  const float* m = M + (size_t)tile * N + n4 * 4;
  float t[MT][A][4];                                  // A^T m : along the rows
#pragma unroll
  for (int j = 0; j < A; ++j) {
    float col[4][A];
#pragma unroll
    for (int i = 0; i < A; ++i) {
      const float4 v = *reinterpret_cast<const float4*>(m + (size_t)(i * A + j) * plane);
      col[0][i] = v.x; col[1][i] = v.y; col[2][i] = v.z; col[3][i] = v.w;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float o[MT];
      Wino<MT>::at(col[e], o);
#pragma unroll
      for (int p = 0; p < MT; ++p) t[p][j][e] = o[p];
    }
  }
  float4 bv = make_float4(0.f, 0.f, 0.f, 0.f);
  if (bias) bv = *reinterpret_cast<const float4*>(bias + n4 * 4);
  const float be[4] = {bv.x, bv.y, bv.z, bv.w};
#pragma unroll
  for (int p = 0; p < MT; ++p) {
    const int oy = ty * MT + p;
    float r[4][MT];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float row[A];
#pragma unroll
      for (int j = 0; j < A; ++j) row[j] = t[p][j][e];
      Wino<MT>::at(row, r[e]);
    }
    if (oy >= H) continue;
#pragma unroll
    for (int q = 0; q < MT; ++q) {
      const int ox = tx * MT + q;
      if (ox >= W) continue;
      const long pix = ((long)b * H + oy) * W + ox;
      float v[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        v[e] = r[e][q] + be[e];
        if (relu) v[e] = fmaxf(v[e], 0.f);
      }
      if (res) {
        const float4 a = *reinterpret_cast<const float4*>(res + pix * res_ld + n4 * 4);
        v[0] += a.x; v[1] += a.y; v[2] += a.z; v[3] += a.w;
      }
      if (res2) {
        const float4 a = *reinterpret_cast<const float4*>(res2 + pix * res2_ld + n4 * 4);
        v[0] += a.x; v[1] += a.y; v[2] += a.z; v[3] += a.w;
      }
      *reinterpret_cast<float4*>(y + pix * y_ld + n4 * 4) = make_float4(v[0], v[1], v[2], v[3]);
    }
  }
  }
}

inline int launch_ok() { return hipGetLastError() == hipSuccess ? PF_OK : PF_ERR_LAUNCH; }

template <int MT>
int run(const pf_conv_params* p, const float* U, int u_rows, int u_kpad, float* V, float* M, hipStream_t st) {
  constexpr int A = MT + 2;
  const int TH = (p->H + MT - 1) / MT, TW = (p->W + MT - 1) / MT;
  const long T = (long)p->B * TH * TW;
  if (T > 0x7fffffffL) return PF_ERR_ARG;
  const long nin = T * (p->Cin / 4), nout = T * (p->Cout / 4);
  hipLaunchKernelGGL(wino_input_kernel<MT>, dim3((unsigned)((nin + 255) / 256)), dim3(256), 0, st, static_cast<const float*>(p->x), p->x_ld,
                     p->B, p->H, p->W, p->Cin, p->relu_in, V, TH, TW, nin, 0L, T);
  if (launch_ok() != PF_OK) return PF_ERR_LAUNCH;
  pf_conv_params q = {};
  q.x_ld = p->Cin; q.B = 1; q.H = 1; q.W = (int)T; q.Cin = p->Cin;
  q.w_rows = u_rows; q.Kpad = u_kpad;
  q.y_ld = p->Cout; q.OH = 1; q.OW = (int)T; q.Cout = p->Cout;
  q.KH = q.KW = 1; q.stride = 1; q.pad = 0; q.act = PF_ACT_NONE; q.shuffle = 1; q.dtype = PF_DTYPE_F32; q.korder = 0;
  q.x = V; q.w = U; q.y = M;                            // the (m+2)^2 transform points = planes of ONE batched GEMM launch
  q.batch = A * A;
  q.x_bstride = T * p->Cin; q.w_bstride = (long)u_rows * u_kpad; q.y_bstride = T * p->Cout;
  const int rc = pf_conv(&q, st);
  if (rc != PF_OK) return rc;
  hipLaunchKernelGGL(wino_output_kernel<MT>, dim3((unsigned)((nout + 255) / 256)), dim3(256), 0, st, M, p->Cout, p->bias,
                     p->act == PF_ACT_RELU ? 1 : 0, static_cast<const float*>(p->res), p->res_ld, static_cast<const float*>(p->res2),
                     p->res2_ld, static_cast<float*>(p->y), p->y_ld, p->B, p->H, p->W, TH, TW, 0L, T);
  return launch_ok();
}

// one event per device shared by every stream of the process (see run_split3); created once per device under a once_flag (two host threads may enter together)
hipEvent_t gemm_token() {
  static hipEvent_t ev[64] = {};
  static std::once_flag once[64];
  int dev = 0;
  hipGetDevice(&dev);
  std::call_once(once[dev & 63], [&] { hipEventCreateWithFlags(&ev[dev & 63], hipEventDisableTiming); });
  return ev[dev & 63];
}

// the three measurement switches of run_split3 (PF_W3_TGRID / PF_W3_GRID / PF_W3_TOKEN; all measured as "does not pay"), read from the environment ONCE
struct W3Switches { int tgrid = 0, cap = 0; bool token = false; };
const W3Switches& w3_switches() {
  static W3Switches sw;
  static std::once_flag once;
  std::call_once(once, [] {
    if (const char* s = getenv("PF_W3_TGRID")) sw.tgrid = atoi(s);
    if (const char* s = getenv("PF_W3_GRID")) sw.cap = atoi(s);
    if (const char* s = getenv("PF_W3_TOKEN")) sw.token = s[0] == '1';
  });
  return sw;
}

// With more than one window, window k's output is written before window k + 1's input (and its one-pixel halo across the seam) is read: x and y
// must not share an element (a single window reads all of x first, like the unwindowed sequence).  Two channel slices of one NHWC buffer (equal
// pixel strides, the engine's concat buffers) share none when y's channels [r, r + Cout) of a row, r = (y - x) mod ld in floats, miss x's [0, Cin)
// without wrapping into the next row; other layouts are refused whenever their byte spans overlap.
bool windows_alias(const pf_conv_params* p) {
  const char* xa = static_cast<const char*>(p->x);
  const char* ya = static_cast<const char*>(p->y);
  const long px = (long)p->B * p->H * p->W;
  const long xb = (px - 1) * p->x_ld * 4 + (long)p->Cin * 4, yb = (px - 1) * p->y_ld * 4 + (long)p->Cout * 4;
  if (!(xa < ya + yb && ya < xa + xb)) return false;
  const long d = (long)(ya - xa);
  if (p->x_ld != p->y_ld || p->x_ld <= 0 || d % 4) return true;
  long r = (d / 4) % p->x_ld;
  if (r < 0) r += p->x_ld;
  return !(r >= p->Cin && r + p->Cout <= p->x_ld);
}

// F(4x4,3x3) with the transform-domain GEMM in split precision: V is written as three bf16 planes, U3 = the three planes of G g G^T
// (chunk-major [3][36][Cin/32][u_rows][32] bf16 = PackedConv.wino_u3, the split3 of packing.winograd_filters), ONE batched pf_gemm_split3 launch (plane = blockIdx.y), M float32.
// cmax_out != nullptr: the output transform also merges the channel maxima of y (of max(y, 0) with cmax_relu) into that uint32 [Cout] buffer, zeroed
// here once before the first window -- the range pass of a following fp16x2 layer (csrc/wino_f16x2_n256.hip wino_output_cmax_kernel).
int run_split3(const pf_conv_params* p, const void* U3, int u_rows, int u_kpad, void* V3, float* M, long window, hipStream_t st,
               unsigned* cmax_out = nullptr, int cmax_relu = 0) {
  constexpr int MT = 4, A = 6;
  const int TH = (p->H + MT - 1) / MT, TW = (p->W + MT - 1) / MT;
  const long Tall = (long)p->B * TH * TW;
  if (Tall > 0x7fffffffL) return PF_ERR_ARG;
  if (window <= 0 || window > Tall) window = Tall;
  // PF_W3_TGRID = n > 0: the transforms run RESIDENT on n CUs (n blocks of 512 threads walking the items) instead of flooding the chip.
  // Overlap of the HBM-bound transforms of one tile batch with the matrix-bound GEMM of the other (two streams; measured, off): the
  // persistent GEMM leaves CUs free (PF_W3_GRID blocks instead of one per CU) and, with PF_W3_TOKEN=1, the big GEMMs of ALL streams are chained
  // through one event in host-issue order, so that two capped GEMMs never compete for the same CUs.
  const W3Switches& sw = w3_switches();
  const int tgrid = sw.tgrid, cap = sw.cap;
  hipEvent_t tok = sw.token ? gemm_token() : nullptr;
  // (x and y of a layer in several windows must not share an element: windows_alias.)  Refused instead of computing from half-overwritten input.
  if (window < Tall && windows_alias(p)) return PF_ERR_ARG;
  if (cmax_out && hipMemsetAsync(cmax_out, 0, (size_t)p->Cout * 4, st) != hipSuccess) return PF_ERR_LAUNCH;
  // TILE WINDOWS (round 5): the layer's tiles go through the three steps `window` tiles at a time, all windows through the SAME V / M arena -- launches
  // of one stream are ordered.  Winograd tiles are independent, so the numbers do not depend on the window.
  for (long t0 = 0; t0 < Tall; t0 += window) {
    const long T = Tall - t0 < window ? Tall - t0 : window;
    const long nin = ((T + 7) / 8) * 8 * (p->Cin / 4), nout = T * (p->Cout / 4);       // (input transform: whole tile octets, see the kernel)
    const bool resident = tgrid > 0 && nin > (long)tgrid * 512 * 4;
    const dim3 gin = resident ? dim3((unsigned)tgrid) : dim3((unsigned)((nin + 255) / 256)), bin = resident ? dim3(512) : dim3(256);
    hipLaunchKernelGGL((wino_input_kernel<MT, true>), gin, bin, 0, st, static_cast<const float*>(p->x), p->x_ld,
                       p->B, p->H, p->W, p->Cin, p->relu_in, static_cast<float*>(V3), TH, TW, nin, t0, T);
    if (launch_ok() != PF_OK) return PF_ERR_LAUNCH;
    pf_conv_params q = {};
    q.x_ld = p->Cin; q.B = 1; q.H = 1; q.W = (int)T; q.Cin = p->Cin;
    q.w_rows = u_rows; q.Kpad = u_kpad;
    q.y_ld = p->Cout; q.OH = 1; q.OW = (int)T; q.Cout = p->Cout;
    q.KH = q.KW = 1; q.stride = 1; q.pad = 0; q.act = PF_ACT_NONE; q.shuffle = 1; q.dtype = PF_DTYPE_BF16; q.out_f32 = 1;
    q.x = V3; q.w = U3; q.y = M;
    q.korder = 6;                                         // V3 and U3 are chunk-major: [plane][point][Cin/32][rows][32]
    q.batch = A * A;                                      // transform points: x / w / y advance by one [T][Cin] / [rows][Kpad] / [T][Cout] block each
    q.x_bstride = (long)A * A * T * p->Cin;               // h / m / l plane strides
    q.w_bstride = (long)A * A * u_rows * u_kpad;
    if (tok) hipStreamWaitEvent(st, tok, 0);
    const int rc = pf_gemm_split3_ex(&q, cap, st);
    if (rc != PF_OK) return rc;
    if (tok) hipEventRecord(tok, st);
    const bool resident_out = tgrid > 0 && nout > (long)tgrid * 512 * 4;
    if (cmax_out) {
      const int rc2 = pf_f16x2::launch_output_cmax(M, p, TH, TW, t0, T, cmax_out, cmax_relu, st);
      if (rc2 != PF_OK) return rc2;
    } else
    hipLaunchKernelGGL(wino_output_kernel<MT>, resident_out ? dim3((unsigned)tgrid) : dim3((unsigned)((nout + 255) / 256)), resident_out ? dim3(512) : dim3(256), 0, st, M,
                       p->Cout, p->bias, p->act == PF_ACT_RELU ? 1 : 0, static_cast<const float*>(p->res), p->res_ld, static_cast<const float*>(p->res2),
                       p->res2_ld, static_cast<float*>(p->y), p->y_ld, p->B, p->H, p->W, TH, TW, t0, T);
    if (!cmax_out && launch_ok() != PF_OK) return PF_ERR_LAUNCH;
  }
  return PF_OK;
}

// fp16x2 form (round 7, csrc/wino_f16x2.hip): per layer call the channel maxima of the input and the scaled filter planes U' (scratch:
// [2][36][Cin/32][u_rows][32] fp16 | int32 [36][u_rows] column exponents | uint32 [Cin] channel maxima), then per window the input transform into
// two fp16 planes, the batched product on three f16 MFMAs per term (pf_gemm_f16x2_points on 192 x 192 tiles, pf_gemm_f16x2_points128 on 128 x 128
// for the layers whose bf16x3 product walks 128-tiles: f16x2_layer_route, or on 160 x 256 tiles where f16x2_layer_tile160 says so:
// csrc/wino_f16x2_t160.hip) and the output transform of run_split3.
// Same windows, same argument rules, one stream.
struct F16x2Scratch { void* u2; int* fexp; unsigned* cmax; };
inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }
F16x2Scratch f16x2_scratch(void* base, int cin, int u_rows) {
  char* b = static_cast<char*>(base);
  const size_t u2 = align256((size_t)2 * 36 * u_rows * cin * 2), fe = align256((size_t)36 * u_rows * 4);
  return {b, reinterpret_cast<int*>(b + u2), reinterpret_cast<unsigned*>(b + u2 + fe)};
}

// the batched GEMM of one window (korder 6: chunk-major V and U' planes)
pf_conv_params f16x2_points_params(const pf_conv_params* p, const void* U2, int u_rows, void* V2, float* M, long T) {
  constexpr int A = 6;
  pf_conv_params q = {};
  q.x_ld = p->Cin; q.B = 1; q.H = 1; q.W = (int)T; q.Cin = p->Cin;
  q.w_rows = u_rows; q.Kpad = p->Cin;
  q.y_ld = p->Cout; q.OH = 1; q.OW = (int)T; q.Cout = p->Cout;
  q.KH = q.KW = 1; q.stride = 1; q.pad = 0; q.act = PF_ACT_NONE; q.shuffle = 1; q.dtype = PF_DTYPE_BF16; q.out_f32 = 1;
  q.x = V2; q.w = U2; q.y = M;
  q.korder = 6;
  q.batch = A * A;
  q.x_bstride = (long)A * A * T * p->Cin;               // h / l plane strides
  q.w_bstride = (long)A * A * u_rows * p->Cin;
  return q;
}

// The GEMM's tile is fixed by the product of the WHOLE layer (one window of all tiles), so every window size of a layer runs the same kernel.
int f16x2_layer_route(const pf_conv_params* p, int u_rows, bool maxima_given = false) {
  const long T = (long)p->B * ((p->H + 3) / 4) * ((p->W + 3) / 4);
  if (T > 0x7fffffffL) return -1;
  pf_conv_params q = f16x2_points_params(p, p->x, u_rows, const_cast<void*>(p->x), static_cast<float*>(p->y), T);
  return pf_gemm_f16x2_points_route_ex(&q, pf_cu_count(), maxima_given ? 1 : 0);
}

}  // namespace

// the 160 x 256 tile form of the product and its per-layer decision (csrc/wino_f16x2_t160.hip)
int pf_f16x2_points160(const pf_conv_params* p, const int* col_exp, int grid_cap, hipStream_t st);
int pf_wino_f16x2_tile(const pf_conv_params& q, int cus);

namespace {

// Like the route, the tile is decided on the product of the WHOLE layer and the CU count: the same kernel, the same bits, for every window size.
bool f16x2_layer_tile160(const pf_conv_params* p, int u_rows) {
  const long T = (long)p->B * ((p->H + 3) / 4) * ((p->W + 3) / 4);
  if (T > 0x7fffffffL) return false;
  const pf_conv_params q = f16x2_points_params(p, p->x, u_rows, const_cast<void*>(p->x), static_cast<float*>(p->y), T);
  return pf_wino_f16x2_tile(q, pf_cu_count()) == 1;
}

// cmax_in != nullptr: the channel maxima of x (uint32 [Cin], of relu(x) when relu_in) are already known -- handed over by the producer's output
// transform -- and the memset + range pass are skipped.  cmax_out / cmax_relu: as run_split3.
// A layer whose whole-layer route is -1 (called directly, or PF_WINO_F16X2_N256 flipped without a new plan) falls to the 192-tile product: correct
// and the same bits, but not where that form was measured to win.
int run_f16x2(const pf_conv_params* p, const float* U, int u_rows, void* V2, float* M, void* scratch, long window, hipStream_t st,
              const unsigned* cmax_in = nullptr, unsigned* cmax_out = nullptr, int cmax_relu = 0) {
  constexpr int MT = 4;
  const bool t128 = f16x2_layer_route(p, u_rows, cmax_in != nullptr) == PF_S3_ROUTE_PERSIST128;
  const bool t160 = f16x2_layer_tile160(p, u_rows);
  const int TH = (p->H + MT - 1) / MT, TW = (p->W + MT - 1) / MT;
  const long Tall = (long)p->B * TH * TW;
  if (Tall > 0x7fffffffL) return PF_ERR_ARG;
  if (window <= 0 || window > Tall) window = Tall;
  if (window < Tall && windows_alias(p)) return PF_ERR_ARG;   // (the alias rule of run_split3)
  const F16x2Scratch sc = f16x2_scratch(scratch, p->Cin, u_rows);
  const float* x = static_cast<const float*>(p->x);
  int rc = PF_OK;
  const unsigned* cmax = cmax_in;
  if (!cmax) {
    if (hipMemsetAsync(sc.cmax, 0, (size_t)p->Cin * 4, st) != hipSuccess) return PF_ERR_LAUNCH;
    rc = pf_f16x2::launch_absmax(x, p->x_ld, (long)p->B * p->H * p->W, p->Cin, p->relu_in, sc.cmax, st);
    if (rc != PF_OK) return rc;
    cmax = sc.cmax;
  }
  if (cmax_out && hipMemsetAsync(cmax_out, 0, (size_t)p->Cout * 4, st) != hipSuccess) return PF_ERR_LAUNCH;
  rc = pf_f16x2::launch_u_split(U, u_rows, p->Cin, cmax, sc.u2, sc.fexp, st);
  if (rc != PF_OK) return rc;
  for (long t0 = 0; t0 < Tall; t0 += window) {
    const long T = Tall - t0 < window ? Tall - t0 : window;
    const long nout = T * (p->Cout / 4);
    rc = pf_f16x2::launch_input(x, p->x_ld, p->B, p->H, p->W, p->Cin, p->relu_in, cmax, V2, TH, TW, t0, T, st);
    if (rc != PF_OK) return rc;
    const pf_conv_params q = f16x2_points_params(p, sc.u2, u_rows, V2, M, T);
    rc = t160 ? pf_f16x2_points160(&q, sc.fexp, 0, st) : t128 ? pf_gemm_f16x2_points128(&q, sc.fexp, 0, st) : pf_gemm_f16x2_points(&q, sc.fexp, 0, st);
    if (rc != PF_OK) return rc;
    if (cmax_out) {
      rc = pf_f16x2::launch_output_cmax(M, p, TH, TW, t0, T, cmax_out, cmax_relu, st);
      if (rc != PF_OK) return rc;
      continue;
    }
    hipLaunchKernelGGL(wino_output_kernel<MT>, dim3((unsigned)((nout + 255) / 256)), dim3(256), 0, st, M, p->Cout, p->bias, p->act == PF_ACT_RELU ? 1 : 0,
                       static_cast<const float*>(p->res), p->res_ld, static_cast<const float*>(p->res2), p->res2_ld, static_cast<float*>(p->y), p->y_ld,
                       p->B, p->H, p->W, TH, TW, t0, T);
    if (launch_ok() != PF_OK) return PF_ERR_LAUNCH;
  }
  return PF_OK;
}

// What every three-step Winograd entry point refuses in `p` (nullptr = accepted): a null p / x / y; tensors (x, y, bias, res, res2) off a 16-byte
// boundary; anything but a float32 3 x 3 / stride 1 / pad 1 layer without pixel shuffle (shuffle != 1) or scale; B, H, W not positive or OH, OW not
// H, W; Cin not a positive multiple of 32, Cout of 8; x_ld / y_ld / res_ld / res2_ld not multiples of 4 or below the channels they hold; an
// activation other than NONE / RELU; 2^31 or more pixels.
const char* wino_layer_refusal(const pf_conv_params* p) {
  if (!p || !p->x || !p->y) return "null tensor";
  if (pf_misaligned(p->x, 16) || pf_misaligned(p->y, 16)) return "misaligned tensor";
  if (const char* e = pf_epilogue_operands(*p, 16, 16)) return e;
  if (p->dtype != PF_DTYPE_F32 || p->KH != 3 || p->KW != 3 || p->stride != 1 || p->pad != 1 || p->shuffle != 1 || p->scale)
    return "float32 3x3 / stride 1 / pad 1 layers without shuffle or scale only";
  if (p->B <= 0 || p->H <= 0 || p->W <= 0 || p->OH != p->H || p->OW != p->W) return "B, H, W must be positive, OH == H, OW == W";
  if (p->Cin <= 0 || p->Cout <= 0 || p->Cin % 32 || p->Cout % 8) return "Cin must be a positive multiple of 32, Cout of 8";
  if (p->x_ld % 4 || p->x_ld < p->Cin || p->y_ld % 4 || p->y_ld < p->Cout) return "x_ld, y_ld must be multiples of 4 and hold the channels";
  if (p->act != PF_ACT_NONE && p->act != PF_ACT_RELU) return "act must be NONE or RELU";
  if ((long)p->B * p->H * p->W >= (1L << 31)) return "too many pixels";
  return nullptr;
}
const char* window_refusal(long window) { return window < 0 || (window > 0 && window % 8) ? "window must be 0 or a positive multiple of 8" : nullptr; }

inline const char* f16x2_why(const pf_conv_params* p) {
  const char* e = wino_layer_refusal(p);
  return e ? e : "window / u_rows / u_kpad / Cin > 8192";
}

// the argument rules of pf_conv_winograd_split3_windowed (U = PackedConv.wino_u: float32 [36][u_rows][Cin])
bool f16x2_args_ok(const pf_conv_params* p, int u_rows, int u_kpad, long window) {
  if (wino_layer_refusal(p) || window_refusal(window) || p->Cin > 8192) return false;
  return u_rows >= p->Cout && u_rows % 16 == 0 && u_kpad == p->Cin;
}

}  // namespace

extern "C" long pf_wino_f16x2_scratch_bytes(int cin, int u_rows) {
  if (cin <= 0 || u_rows <= 0) return 0;
  return (long)(align256((size_t)2 * 36 * u_rows * cin * 2) + align256((size_t)36 * u_rows * 4) + align256((size_t)cin * 4));
}

// 1 when the layer runs the fp16x2 product: the arguments qualify and the bf16x3 GEMM of the WHOLE layer (all tiles in one window) would take one
// of the persistent kernels -- 192 x 192 tiles, or 128 x 128 (the N = 256 layers; csrc/wino_f16x2_n256.hip).  The rule is pf_gemm_f16x2_points_route
// (csrc/gemm_split3.hip).  The decision does not depend on the window, so every window size of a layer computes the same bits.
extern "C" int pf_conv_winograd_f16x2_supported(const pf_conv_params* p, int u_rows, int u_kpad, long window) {
  if (!f16x2_args_ok(p, u_rows, u_kpad, window)) return 0;
  return f16x2_layer_route(p, u_rows) >= 0 ? 1 : 0;
}

// the same for a call that will hand in the channel maxima (cmax_in): the rule of pf_gemm_f16x2_points_route_ex
extern "C" int pf_conv_winograd_f16x2_supported_ex(const pf_conv_params* p, int u_rows, int u_kpad, long window, int maxima_given) {
  if (!f16x2_args_ok(p, u_rows, u_kpad, window)) return 0;
  return f16x2_layer_route(p, u_rows, maxima_given != 0) >= 0 ? 1 : 0;
}

extern "C" int pf_conv_winograd_f16x2_windowed(const pf_conv_params* p, const void* U, int u_rows, int u_kpad, void* V2, void* M, void* scratch,
                                               long window, void* stream) {
  if (!U || !V2 || !M || !scratch) return pf_refuse("pf_conv_winograd_f16x2_windowed", "null pointer");
  if (pf_misaligned(U, 16) || pf_misaligned(V2, 16) || pf_misaligned(M, 16) || pf_misaligned(scratch, 16)) return pf_refuse("pf_conv_winograd_f16x2_windowed", "misaligned pointer");
  if (!f16x2_args_ok(p, u_rows, u_kpad, window)) return pf_refuse("pf_conv_winograd_f16x2_windowed", f16x2_why(p));
  return run_f16x2(p, static_cast<const float*>(U), u_rows, V2, static_cast<float*>(M), scratch, window, ST(stream));
}

// the same call with the range pass handed between layers: cmax_in = the channel maxima of x as the producer's output transform merged them
// (uint32 [Cin] float bits; of relu(x) when p->relu_in), or null = run the range pass; cmax_out = where this layer's output transform merges the
// maxima of y (uint32 [Cout]; of max(y, 0) when cmax_out_relu), or null.  cmax_out must not be the buffer cmax_in points to.
extern "C" int pf_conv_winograd_f16x2_windowed_ex(const pf_conv_params* p, const void* U, int u_rows, int u_kpad, void* V2, void* M, void* scratch,
                                                  long window, const void* cmax_in, void* cmax_out, int cmax_out_relu, void* stream) {
  if (!U || !V2 || !M || !scratch) return pf_refuse("pf_conv_winograd_f16x2_windowed_ex", "null pointer");
  if (pf_misaligned(U, 16) || pf_misaligned(V2, 16) || pf_misaligned(M, 16) || pf_misaligned(scratch, 16) || pf_misaligned(cmax_in, 4) || pf_misaligned(cmax_out, 4))
    return pf_refuse("pf_conv_winograd_f16x2_windowed_ex", "misaligned pointer");
  if (!f16x2_args_ok(p, u_rows, u_kpad, window)) return pf_refuse("pf_conv_winograd_f16x2_windowed_ex", f16x2_why(p));
  if (cmax_in && cmax_in == cmax_out) return pf_refuse("pf_conv_winograd_f16x2_windowed_ex", "cmax_out must not be cmax_in");
  return run_f16x2(p, static_cast<const float*>(U), u_rows, V2, static_cast<float*>(M), scratch, window, ST(stream),
                   static_cast<const unsigned*>(cmax_in), static_cast<unsigned*>(cmax_out), cmax_out_relu);
}

extern "C" int pf_wino_absmax(const void* x, int x_ld, long P, int C, int relu_in, void* cmax, void* stream) {
  if (!x || !cmax || pf_misaligned(x, 16) || pf_misaligned(cmax, 4)) return pf_refuse("pf_wino_absmax", "null or misaligned pointer");
  if (P <= 0 || C <= 0 || C % 4 || x_ld < C || x_ld % 4) return pf_refuse("pf_wino_absmax", "P must be positive, C a positive multiple of 4, x_ld a multiple of 4 >= C");
  return pf_f16x2::launch_absmax(static_cast<const float*>(x), x_ld, P, C, relu_in, static_cast<unsigned*>(cmax), ST(stream));
}

extern "C" int pf_conv_winograd_split3(const pf_conv_params* p, const void* U3, int u_rows, int u_kpad, void* V3, void* M, void* stream) {
  if (!U3 || !V3 || !M) return pf_refuse("pf_conv_winograd_split3", "null pointer");
  if (pf_misaligned(U3, 16) || pf_misaligned(V3, 16) || pf_misaligned(M, 16)) return pf_refuse("pf_conv_winograd_split3", "misaligned pointer");
  if (const char* e = wino_layer_refusal(p)) return pf_refuse("pf_conv_winograd_split3", e);
  if (u_rows < p->Cout || u_kpad != p->Cin) return pf_refuse("pf_conv_winograd_split3", "u_rows must be >= Cout, u_kpad == Cin");       // (chunk-major planes are dense in K)
  return run_split3(p, U3, u_rows, u_kpad, V3, static_cast<float*>(M), 0, ST(stream));
}

// the same layer `window` Winograd tiles at a time (0 / >= all tiles: one window): V3 / M are arenas for ONE window -- 3 x 36 x ceil8(window) x Cin bf16
// and 36 x window x Cout float32.  Identical results for every window (tiles are independent).
extern "C" int pf_conv_winograd_split3_windowed(const pf_conv_params* p, const void* U3, int u_rows, int u_kpad, void* V3, void* M, long window, void* stream) {
  if (!U3 || !V3 || !M) return pf_refuse("pf_conv_winograd_split3_windowed", "null pointer");
  if (pf_misaligned(U3, 16) || pf_misaligned(V3, 16) || pf_misaligned(M, 16)) return pf_refuse("pf_conv_winograd_split3_windowed", "misaligned pointer");
  if (const char* e = wino_layer_refusal(p)) return pf_refuse("pf_conv_winograd_split3_windowed", e);
  if (const char* e = window_refusal(window)) return pf_refuse("pf_conv_winograd_split3_windowed", e);
  if (u_rows < p->Cout || u_kpad != p->Cin) return pf_refuse("pf_conv_winograd_split3_windowed", "u_rows must be >= Cout, u_kpad == Cin");
  return run_split3(p, U3, u_rows, u_kpad, V3, static_cast<float*>(M), window, ST(stream));
}

// the same layer as the PRODUCER of an fp16x2 layer's range pass: its output transform merges the channel maxima of y into cmax_out (uint32 [Cout])
extern "C" int pf_conv_winograd_split3_windowed_ex(const pf_conv_params* p, const void* U3, int u_rows, int u_kpad, void* V3, void* M, long window,
                                                   void* cmax_out, int cmax_out_relu, void* stream) {
  if (!U3 || !V3 || !M) return pf_refuse("pf_conv_winograd_split3_windowed_ex", "null pointer");
  if (pf_misaligned(U3, 16) || pf_misaligned(V3, 16) || pf_misaligned(M, 16) || pf_misaligned(cmax_out, 4)) return pf_refuse("pf_conv_winograd_split3_windowed_ex", "misaligned pointer");
  if (const char* e = wino_layer_refusal(p)) return pf_refuse("pf_conv_winograd_split3_windowed_ex", e);
  if (const char* e = window_refusal(window)) return pf_refuse("pf_conv_winograd_split3_windowed_ex", e);
  if (u_rows < p->Cout || u_kpad != p->Cin) return pf_refuse("pf_conv_winograd_split3_windowed_ex", "u_rows must be >= Cout, u_kpad == Cin");
  return run_split3(p, U3, u_rows, u_kpad, V3, static_cast<float*>(M), window, ST(stream), static_cast<unsigned*>(cmax_out), cmax_out_relu);
}

extern "C" int pf_conv_winograd(const pf_conv_params* p, int m, const void* U, int u_rows, int u_kpad, void* V, void* M, void* stream) {
  if (!U || !V || !M) return pf_refuse("pf_conv_winograd", "null pointer");
  if (pf_misaligned(U, 16) || pf_misaligned(V, 16) || pf_misaligned(M, 16)) return pf_refuse("pf_conv_winograd", "misaligned pointer");
  if (const char* e = wino_layer_refusal(p)) return pf_refuse("pf_conv_winograd", e);
  if (m != 2 && m != 4) return pf_refuse("pf_conv_winograd", "m must be 2 or 4");
  if (u_rows < p->Cout || u_kpad < p->Cin || u_kpad % 32) return pf_refuse("pf_conv_winograd", "u_rows must be >= Cout, u_kpad a multiple of 32 >= Cin");
  if (m == 2) return run<2>(p, static_cast<const float*>(U), u_rows, u_kpad, static_cast<float*>(V), static_cast<float*>(M), ST(stream));
  if (m == 4) return run<4>(p, static_cast<const float*>(U), u_rows, u_kpad, static_cast<float*>(V), static_cast<float*>(M), ST(stream));
  return PF_ERR_ARG;
}
