// Training-side augmentations of the reference's UnrealStereo4kDataset (estimator/datasets/u4k_dataset.py:121-134,
// transformers/augmentations.py) on the device.  The host draws every random number first (datasets.py); the two launches here are pure
// functions of the uploaded sample and those numbers:
//
//   pf_aug_image_u8_to_f32   uint8 [H][W][3] in file order (B, G, R)  ->  float32 [3][H][W] (R, G, B):
//       aug_rotate   Image.rotate(angle, resample=BILINEAR) of Pillow on an RGB image: affine_transform + bilinear_filter32RGB of
//                    Geometry.c, every product and sum its own double operation (the pragma below: a fused multiply-add moves the floor
//                    or the truncation at rare pixels), the blend truncated to a byte;
//       the flip     output (y, x) samples the rotated image at (W - 1 - x, y);
//       numpy        float32(v) / 255.0f; with the colour augmentation  p = v ** float32(gamma) (evaluated in double, rounded once),
//                    p * float32(brightness), float32(double(p) * colour[c]) -- numpy forms the product of a float32 array with a float64
//                    array in double -- and the clip to [0, 1].
//   pf_aug_planes_nearest    one or two float32 [H][W] planes (depth, disparity)  ->  the same, rotated by Image.rotate(angle,
//       resample=NEAREST) on mode 'F' (the 16.16 fixed-point path of ImagingTransformAffine) and flipped; 0 outside the source.
//
// Both are gather-and-stream: one thread makes four adjacent output pixels of a row and writes them with one 16-byte store per plane when
// W % 4 == 0 (every row of a 16-byte aligned plane then starts on a 16-byte boundary), float by float otherwise.  No LDS, no scratch; the
// taps of adjacent pixels are adjacent bytes, so the loads of a wave stay inside a few cache lines per source row.
#include "pf_common.h"
#include "../../include/pf_hip.h"

#pragma clang fp contract(off)

namespace {

inline int grid_for(long n, int block) {
  long g = (n + block - 1) / block;
  return (int)(g > 8192 ? 8192 : (g < 1 ? 1 : g));
}
inline int ok() { return hipGetLastError() == hipSuccess ? PF_OK : PF_ERR_LAUNCH; }
#define ST(s) reinterpret_cast<hipStream_t>(s)

struct ImageArgs {
  double m[6];       // Image.rotate's matrix
  double colour[3];  // per RGB channel
  float gamma, brightness;
  int flip;
};

struct PlaneArgs {
  long a[6];         // the 16.16 integers
  int flip;
};

__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// the three bytes of the rotated image at output position (x, y), in file order
__device__ __forceinline__ void rotated_pixel(const uint8_t* __restrict__ img, int H, int W, const ImageArgs& p, int x, int y, int out[3]) {
  const double xc = (double)x + 0.5, yc = (double)y + 0.5;
  const double xs = p.m[0] * xc + p.m[1] * yc + p.m[2];
  const double ys = p.m[3] * xc + p.m[4] * yc + p.m[5];
  out[0] = out[1] = out[2] = 0;
  if (xs < 0.0 || xs >= (double)W || ys < 0.0 || ys >= (double)H) return;      // before the half-pixel shift
  const double xin = xs - 0.5, yin = ys - 0.5;
  const double fx = floor(xin), fy = floor(yin);
  const double dx = xin - fx, dy = yin - fy;
  const int x0 = (int)fx, y0 = (int)fy;                                         // >= -1 and < W, H: inside int
  const int xa = clampi(x0, W - 1) * 3, xb = clampi(x0 + 1, W - 1) * 3;
  const uint8_t* r0 = img + (long)clampi(y0, H - 1) * W * 3;
  const bool below = y0 + 1 >= 0 && y0 + 1 < H;
  const uint8_t* r1 = img + (long)(below ? y0 + 1 : 0) * W * 3;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const double a = (double)r0[xa + c], b = (double)r0[xb + c];
    const double v1 = a + (b - a) * dx;
    double v2 = v1;
    if (below) {
      const double e = (double)r1[xa + c], f = (double)r1[xb + c];
      v2 = e + (f - e) * dx;
    }
    out[c] = (int)(v1 + (v2 - v1) * dy);                                        // truncated, not rounded
  }
}

template <bool COLOUR>
__device__ __forceinline__ float unit_value(int byte, int c, const ImageArgs& p) {
  float v = __fdiv_rn((float)byte, 255.0f);
  if (COLOUR) {
    v = (float)pow((double)v, (double)p.gamma);
    v = v * p.brightness;
    v = (float)((double)v * p.colour[c]);
    v = fminf(fmaxf(v, 0.0f), 1.0f);
  }
  return v;
}

template <bool COLOUR, bool VEC>
__global__ __launch_bounds__(256) void aug_image_kernel(const uint8_t* __restrict__ img, int H, int W, ImageArgs p, float* __restrict__ out) {
  const int gw = (W + 3) >> 2;                                // groups of four pixels per row
  const long groups = (long)H * gw, plane = (long)H * W;
  for (long g = (long)blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += (long)gridDim.x * blockDim.x) {
    const int y = (int)(g / gw), x4 = (int)(g - (long)y * gw) << 2;
    float v[3][4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int x = x4 + j < W ? x4 + j : W - 1;             // past the row's end: a valid pixel again, never stored
      int bgr[3];
      rotated_pixel(img, H, W, p, p.flip ? W - 1 - x : x, y, bgr);
#pragma unroll
      for (int c = 0; c < 3; ++c) v[c][j] = unit_value<COLOUR>(bgr[2 - c], c, p);
    }
    float* o = out + (long)y * W + x4;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      if (VEC) {                                              // W % 4 == 0: the group is whole and 16-byte aligned
        *reinterpret_cast<float4*>(o + c * plane) = make_float4(v[c][0], v[c][1], v[c][2], v[c][3]);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (x4 + j < W) o[c * plane + j] = v[c][j];
      }
    }
  }
}

template <bool TWO, bool VEC>
__global__ __launch_bounds__(256) void aug_planes_kernel(const float* __restrict__ s0, const float* __restrict__ s1, int H, int W, PlaneArgs p,
                                                         float* __restrict__ d0, float* __restrict__ d1) {
  const int gw = (W + 3) >> 2;
  const long groups = (long)H * gw;
  for (long g = (long)blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += (long)gridDim.x * blockDim.x) {
    const int y = (int)(g / gw), x4 = (int)(g - (long)y * gw) << 2;
    float u[4], w[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int x = x4 + j;
      const long xp = p.flip ? W - 1 - x : x;
      const long sx = (p.a[2] + xp * p.a[0] + (long)y * p.a[1]) >> 16;      // arithmetic shift: floor
      const long sy = (p.a[5] + xp * p.a[3] + (long)y * p.a[4]) >> 16;
      const bool inside = x < W && sx >= 0 && sx < W && sy >= 0 && sy < H;
      const long at = inside ? sy * W + sx : 0;
      u[j] = inside ? s0[at] : 0.0f;
      w[j] = TWO && inside ? s1[at] : 0.0f;
    }
    const long o = (long)y * W + x4;
    if (VEC) {
      *reinterpret_cast<float4*>(d0 + o) = make_float4(u[0], u[1], u[2], u[3]);
      if (TWO) *reinterpret_cast<float4*>(d1 + o) = make_float4(w[0], w[1], w[2], w[3]);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (x4 + j < W) {
          d0[o + j] = u[j];
          if (TWO) d1[o + j] = w[j];
        }
      }
    }
  }
}

bool overlap(const void* a, long na, const void* b, long nb) {
  const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
  return a && b && x < y + (uintptr_t)nb && y < x + (uintptr_t)na;
}

}  // namespace

extern "C" int pf_aug_image_u8_to_f32(const unsigned char* img, int H, int W, const double* m, int flip, int colour_on, float gamma,
                                      float brightness, const double* colour, float* out, void* stream) {
  if (!img || !out || !m || H <= 0 || W <= 0) return PF_ERR_ARG;
  if ((long)H * W > 0x7fffffffL || W > 0x7fffffff / 3) return PF_ERR_ARG;   // a tap's byte offset inside its row stays inside int
  if (colour_on && !colour) return PF_ERR_ARG;
  if (reinterpret_cast<uintptr_t>(out) & 15u) return PF_ERR_ARG;        // 16-byte stores
  const long n = (long)H * W;
  if (overlap(img, 3 * n, out, 12 * n)) return PF_ERR_ARG;
  ImageArgs p;
  for (int i = 0; i < 6; ++i) {
    if (m[i] - m[i] != 0.0) return PF_ERR_ARG;                          // NaN or infinite
    p.m[i] = m[i];
  }
  for (int c = 0; c < 3; ++c) p.colour[c] = colour_on ? colour[c] : 1.0;
  p.gamma = gamma;
  p.brightness = brightness;
  p.flip = flip ? 1 : 0;
  const int grid = grid_for((long)H * ((W + 3) / 4), 256);
  const bool vec = W % 4 == 0;
  if (colour_on) {
    if (vec) hipLaunchKernelGGL((aug_image_kernel<true, true>), dim3(grid), dim3(256), 0, ST(stream), img, H, W, p, out);
    else hipLaunchKernelGGL((aug_image_kernel<true, false>), dim3(grid), dim3(256), 0, ST(stream), img, H, W, p, out);
  } else {
    if (vec) hipLaunchKernelGGL((aug_image_kernel<false, true>), dim3(grid), dim3(256), 0, ST(stream), img, H, W, p, out);
    else hipLaunchKernelGGL((aug_image_kernel<false, false>), dim3(grid), dim3(256), 0, ST(stream), img, H, W, p, out);
  }
  return ok();
}

extern "C" int pf_aug_planes_nearest(const float* src0, const float* src1, int H, int W, const int* a, int flip, float* dst0, float* dst1,
                                     void* stream) {
  if (!src0 || !dst0 || !a || H <= 0 || W <= 0 || (src1 == nullptr) != (dst1 == nullptr)) return PF_ERR_ARG;
  if ((long)H * W > 0x7fffffffL) return PF_ERR_ARG;
  if ((reinterpret_cast<uintptr_t>(dst0) | reinterpret_cast<uintptr_t>(dst1)) & 15u) return PF_ERR_ARG;   // 16-byte stores
  const long nb = 4L * H * W;
  if (overlap(src0, nb, dst0, nb) || overlap(src0, nb, dst1, nb) || overlap(src1, nb, dst0, nb) || overlap(src1, nb, dst1, nb) ||
      overlap(dst0, nb, dst1, nb))
    return PF_ERR_ARG;
  PlaneArgs p;
  for (int i = 0; i < 6; ++i) p.a[i] = a[i];                            // 32-bit terms times coordinates below 2^31: the sums stay inside 64 bits
  p.flip = flip ? 1 : 0;
  const int grid = grid_for((long)H * ((W + 3) / 4), 256);
  const bool vec = W % 4 == 0;
  if (src1) {
    if (vec) hipLaunchKernelGGL((aug_planes_kernel<true, true>), dim3(grid), dim3(256), 0, ST(stream), src0, src1, H, W, p, dst0, dst1);
    else hipLaunchKernelGGL((aug_planes_kernel<true, false>), dim3(grid), dim3(256), 0, ST(stream), src0, src1, H, W, p, dst0, dst1);
  } else {
    if (vec) hipLaunchKernelGGL((aug_planes_kernel<false, true>), dim3(grid), dim3(256), 0, ST(stream), src0, src1, H, W, p, dst0, dst1);
    else hipLaunchKernelGGL((aug_planes_kernel<false, false>), dim3(grid), dim3(256), 0, ST(stream), src0, src1, H, W, p, dst0, dst1);
  }
  return ok();
}
