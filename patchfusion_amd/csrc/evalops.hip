// Evaluation side of the output stage: what the reference's evaluation loop (tools/test.py -> Tester.run ->
// dataset.get_metrics) still did on the CPU after io.hip.
//   * depth_boundaries_kernel - estimator/utils/image_ops.py:25-36 get_boundaries (duplicated at metric.py:74-85): threshold of the
//                               four neighbour differences + cv2.dilate by a k x k box of ones, one launch.  OpenCV is not installed
//                               where this was written: the anchor / border rule below is derived from cv2.dilate's documented
//                               definition (anchor (k/2, k/2), out-of-image pixels never raise a maximum) -- parity unpinned against
//                               OpenCV itself, pinned by KATs (tests/test_eval_side_gpu.py).
//   * colorize_bgr_kernel     - the colour mapping of io.hip's colorize_kernel written as 3-byte BGR pixels: colorize_infer_pfv1
//                               (color.py:8-25, `value[:, :, :3][..., ::-1]`) and the tester's `colorize(...)[:, :, [2, 1, 0]]`
//                               (tester.py:69-71) are the same bytes.
#include "pf_common.h"
#include "../../include/pf_hip.h"

namespace {

inline int grid_for(long n, int block) {
  long g = (n + block - 1) / block;
  return (int)(g > 8192 ? 8192 : (g < 1 ? 1 : g));
}
inline int ok() { return hipGetLastError() == hipSuccess ? PF_OK : PF_ERR_LAUNCH; }
#define ST(s) reinterpret_cast<hipStream_t>(s)

// ------------------------------------------------------------------------------------------------
// get_boundaries.  One block makes a BD_TH x BD_TW tile of the output.  With a = k/2 the output pixel (Y, X) is the maximum of the
// edge plane over rows Y-a .. Y-a+k-1 and columns X-a .. X-a+k-1, so the block needs the edge plane on (BD_TH+k-1) x (BD_TW+k-1)
// pixels starting at (tile origin - a), and the disparity one pixel further out on every side.  Three LDS stages:
//   s  [EH+2][EW+2] float   disparity; NaN outside the image: every comparison with NaN is false, which is both "a neighbour outside
//                           the image does not count" and "an edge pixel outside the image does not contribute"
//   e  [EH][EWP]    byte    |centre - neighbour| > th for any of the four neighbours (float32 difference like numpy)
//   rm [EH][BD_TW]  byte    maximum of e over the k columns of the window
// and the column maximum of rm over the k rows goes to HBM as 0.0f / 1.0f.  dilation 0 runs as k = 1 (a 1 x 1 box is the identity).
// The disparity is read once apart from halos and the edge plane written once: 8 B per pixel.
// ------------------------------------------------------------------------------------------------
constexpr int BD_TW = 64, BD_TH = 32, BD_THREADS = 256, BD_MAX_K = 32;

__host__ __device__ inline int bd_sw(int k) { return BD_TW + k + 1; }              // floats per row of s (EW + 2)
__host__ __device__ inline int bd_ewp(int k) { return (BD_TW + k - 1 + 3) & ~3; }  // bytes per row of e
__host__ __device__ inline int bd_s_bytes(int k) { return ((BD_TH + k + 1) * bd_sw(k) * 4 + 15) & ~15; }
__host__ __device__ inline int bd_e_bytes(int k) { return ((BD_TH + k - 1) * bd_ewp(k) + 15) & ~15; }
inline int bd_lds_bytes(int k) { return bd_s_bytes(k) + bd_e_bytes(k) + (BD_TH + k - 1) * BD_TW; }

__global__ __launch_bounds__(BD_THREADS) void depth_boundaries_kernel(const float* __restrict__ disp, int H, int W, float th, int k,
                                                                      float* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char bd_lds[];
  const int a = k >> 1, EH = BD_TH + k - 1, EW = BD_TW + k - 1, SW = bd_sw(k), EWP = bd_ewp(k);
  float* s = reinterpret_cast<float*>(bd_lds);
  unsigned char* e = bd_lds + bd_s_bytes(k);
  unsigned char* rm = e + bd_e_bytes(k);
  const long plane = (long)blockIdx.z * H * W;           // 64-bit plane base, 32-bit indices inside the plane
  const float* __restrict__ src = disp + plane;
  float* __restrict__ dst = out + plane;
  const int ty0 = blockIdx.y * BD_TH, tx0 = blockIdx.x * BD_TW;
  const int sy0 = ty0 - a - 1, sx0 = tx0 - a - 1;          // image position of s[0][0]
  const float qnan = __uint_as_float(0x7fc00000u);
  const int tid = threadIdx.x;

  for (int i = tid; i < (EH + 2) * SW; i += BD_THREADS) {
    const int r = i / SW, c = i - r * SW;
    const int gy = sy0 + r, gx = sx0 + c;
    s[i] = ((unsigned)gy < (unsigned)H && (unsigned)gx < (unsigned)W) ? src[gy * W + gx] : qnan;
  }
  __syncthreads();
  for (int i = tid; i < EH * EW; i += BD_THREADS) {
    const int r = i / EW, c = i - r * EW;
    const float* p = s + (r + 1) * SW + (c + 1);
    const float v = p[0];
    const bool hit = fabsf(v - p[-SW]) > th || fabsf(v - p[SW]) > th || fabsf(v - p[-1]) > th || fabsf(v - p[1]) > th;
    e[r * EWP + c] = hit ? 1 : 0;
  }
  __syncthreads();
  for (int i = tid; i < EH * BD_TW; i += BD_THREADS) {
    const int r = i / BD_TW, x = i - r * BD_TW;
    const unsigned char* p = e + r * EWP + x;
    unsigned int m = 0;
    for (int j = 0; j < k; ++j) m |= p[j];
    rm[i] = (unsigned char)m;
  }
  __syncthreads();
  for (int i = tid; i < BD_TH * BD_TW; i += BD_THREADS) {
    const int y = i / BD_TW, x = i - y * BD_TW;
    const int gy = ty0 + y, gx = tx0 + x;
    if (gy >= H || gx >= W) continue;
    const unsigned char* p = rm + i;
    unsigned int m = 0;
    for (int j = 0; j < k; ++j) m |= p[j * BD_TW];
    dst[gy * W + gx] = m ? 1.f : 0.f;
  }
}

// ------------------------------------------------------------------------------------------------
// colour index of one value: the arithmetic of io.hip's colorize_kernel (color.py:130-135 + matplotlib Colormap.__call__(bytes=True))
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t colour_of(float v, bool invalid, float vmin, float vmax, float den, float fN, int N,
                                              const uint32_t* __restrict__ lut, uint32_t background) {
  if (invalid) return background;
  float x = vmin != vmax ? __fdiv_rn(v - vmin, den) : v * 0.f;
  int idx;
  if (x != x) {
    idx = N + 2;
  } else {
    x = x * fN;
    if (x < 0.f) idx = N;             // under
    else if (x == fN) idx = N - 1;
    else if (x > fN) idx = N + 1;     // over
    else idx = (int)x;
  }
  return lut[idx];
}

// RGBA word (R in the low byte) -> B | G<<8 | R<<16
__device__ __forceinline__ uint32_t bgr_of(uint32_t c) { return ((c >> 16) & 255u) | (c & 0xff00u) | ((c & 255u) << 16); }

// four pixels = twelve bytes = three aligned words per thread; the last n % 4 pixels byte by byte
__global__ __launch_bounds__(256) void colorize_bgr_kernel(const float* __restrict__ depth, long n, const float* __restrict__ vmm,
                                                           const uint32_t* __restrict__ lut, int N, float invalid, int use_invalid,
                                                           const uint8_t* __restrict__ imask, uint32_t background, uint8_t* __restrict__ out) {
  const float vmin = vmm[0], vmax = vmm[1];
  const float den = vmax - vmin;
  const float fN = (float)N;
  const long groups = (n + 3) / 4;
  for (long g = (long)blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += (long)gridDim.x * blockDim.x) {
    const long i0 = g * 4;
    uint32_t c[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const long i = i0 + j < n ? i0 + j : n - 1;
      const float v = depth[i];
      const bool inval = imask ? imask[i] != 0 : (use_invalid && v == invalid);
      c[j] = bgr_of(colour_of(v, inval, vmin, vmax, den, fN, N, lut, background));
    }
    if (i0 + 4 <= n) {
      uint32_t* o = reinterpret_cast<uint32_t*>(out + i0 * 3);
      o[0] = c[0] | (c[1] << 24);
      o[1] = (c[1] >> 8) | (c[2] << 16);
      o[2] = (c[2] >> 16) | (c[3] << 8);
    } else {
      for (int j = 0; i0 + j < n; ++j) {
        uint8_t* o = out + (i0 + j) * 3;
        o[0] = (uint8_t)c[j];
        o[1] = (uint8_t)(c[j] >> 8);
        o[2] = (uint8_t)(c[j] >> 16);
      }
    }
  }
}

}  // namespace

extern "C" int pf_depth_boundaries(const float* disp, int planes, int H, int W, float th, int dilation, float* edges, void* stream) {
  if (!disp || !edges || planes <= 0 || planes > 65535 || H <= 0 || W <= 0) return PF_ERR_ARG;
  if (dilation < 0 || dilation > BD_MAX_K) return PF_ERR_ARG;        // no silent fall-back beyond the LDS tile
  if ((long)H * W > 0x7fffffffL) return PF_ERR_ARG;                  // 32-bit indices inside a plane
  const int gy = (H + BD_TH - 1) / BD_TH, gx = (W + BD_TW - 1) / BD_TW;
  if (gy > 65535) return PF_ERR_ARG;
  const int k = dilation > 0 ? dilation : 1;
  hipLaunchKernelGGL(depth_boundaries_kernel, dim3(gx, gy, planes), dim3(BD_THREADS), bd_lds_bytes(k), ST(stream), disp, H, W, th, k, edges);
  return ok();
}

extern "C" int pf_colorize_f32_ex(const float* depth, long n, const float* vmin_vmax, const uint8_t* lut_rgba, int N, float invalid_val,
                                  int use_invalid, const uint8_t* invalid_mask, uint32_t background_rgba, int layout, uint8_t* out,
                                  void* stream) {
  if (layout == PF_COLOR_RGBA)
    return pf_colorize_f32(depth, n, vmin_vmax, lut_rgba, N, invalid_val, use_invalid, invalid_mask, background_rgba, out, stream);
  if (layout != PF_COLOR_BGR) return PF_ERR_ARG;
  if (!depth || !vmin_vmax || !lut_rgba || !out || n <= 0 || N <= 0) return PF_ERR_ARG;
  if (reinterpret_cast<uintptr_t>(out) & 3u) return PF_ERR_ARG;      // word stores
  hipLaunchKernelGGL(colorize_bgr_kernel, dim3(grid_for((n + 3) / 4, 256)), dim3(256), 0, ST(stream), depth, n, vmin_vmax,
                     reinterpret_cast<const uint32_t*>(lut_rgba), N, invalid_val, use_invalid, invalid_mask, background_rgba, out);
  return ok();
}
