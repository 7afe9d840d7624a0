// Ground-truth side of the evaluation loop: the payload of a depth / disparity file, uploaded as it lies on disk, becomes the float32
// depth plane (and, where the dataset has one, the plane the reference hands to get_boundaries) in one streaming launch.  What the
// reference does on the host with numpy (estimator/datasets/general_dataset.py:60-143 DepthMap, u4k_dataset.py:118-119,168):
//   u4k         .npy disparity, half / float / double     x = float32(src);  depth = df / x;                       edge source x
//   mid         PFM float, either byte order, bottom-up   depth = (fb / (x + doffs)) / 1000, 0 where x == +inf;    edge source x, +inf -> 0
//   eth3d       raw little-endian float                   depth = x with NaN, +inf, -inf -> 0                      (edge source = depth)
//   gta         16- (or 8-) bit grey                      depth = float32(s) / 256                                 (edge source = depth)
//   cityscapes  16- (or 8-) bit grey                      d = s > 0 ? (s - 1) / 256 : 0;  depth = c / d, NaN and +-inf -> 0  (the same)
//   raw         half / float / double                     depth = float32(src): read_pfm and read_npy
// df, fb, doffs and c arrive already rounded to float32 (numpy rounds a Python float to the array's type first); every +, - and / below is
// ONE correctly rounded float32 operation (__fdiv_rn; nothing here can contract into an FMA) and hipcc's default mode keeps denormals, so
// the planes equal numpy's bit for bit (NaN payloads aside).  Edges are pf_depth_boundaries on the edge-source plane.
//
// One thread makes four consecutive output pixels: one 16-byte store per plane.  The source is read as one vector of four samples when
// that vector is aligned and inside one source row -- always without a flip, with a flip only when W % 4 == 0 -- and sample by sample
// otherwise (rows of an arbitrary W start at any sample, and a flipped row order breaks the run of four at a row end).  The last
// H * W % 4 pixels are written one float at a time.
#include "pf_common.h"
#include "../../include/pf_hip.h"

namespace {

inline int grid_for(long n, int block) {
  long g = (n + block - 1) / block;
  return (int)(g > 8192 ? 8192 : (g < 1 ? 1 : g));
}
inline int ok() { return hipGetLastError() == hipSuccess ? PF_OK : PF_ERR_LAUNCH; }
#define ST(s) reinterpret_cast<hipStream_t>(s)

// the sample as it lies in the file: its bits, and their conversion to float32
template <int KIND> struct Sample;
template <> struct Sample<PF_GT_F16> {
  typedef uint16_t raw;
  __device__ static __forceinline__ float get(raw r, bool swap) {
    if (swap) r = (raw)((r << 8) | (r >> 8));
    _Float16 h;
    __builtin_memcpy(&h, &r, 2);
    return (float)h;                                          // exact, half denormals included
  }
};
template <> struct Sample<PF_GT_F32> {
  typedef uint32_t raw;
  __device__ static __forceinline__ float get(raw r, bool swap) { return __uint_as_float(swap ? __builtin_bswap32(r) : r); }
};
template <> struct Sample<PF_GT_F64> {
  typedef uint64_t raw;
  __device__ static __forceinline__ float get(raw r, bool swap) {
    if (swap) r = __builtin_bswap64(r);
    double d;
    __builtin_memcpy(&d, &r, 8);
    return (float)d;                                          // v_cvt_f32_f64: round to nearest even, denormal results kept
  }
};
template <> struct Sample<PF_GT_U8> {
  typedef uint8_t raw;
  __device__ static __forceinline__ float get(raw r, bool) { return (float)r; }
};
template <> struct Sample<PF_GT_U16> {
  typedef uint16_t raw;
  __device__ static __forceinline__ float get(raw r, bool) { return (float)r; }
};

template <typename R> struct alignas(sizeof(R) * 4 < 16 ? sizeof(R) * 4 : 16) Raw4 { R v[4]; };

__device__ __forceinline__ float finite_or_zero(float v) { return (__float_as_uint(v) & 0x7f800000u) == 0x7f800000u ? 0.f : v; }

// one pixel: x = float32(sample) -> depth d and edge source e (e is unused where the edge source is the depth itself)
__device__ __forceinline__ void convert(int mode, float x, float a, float b, float& d, float& e) {
  const float inf = __uint_as_float(0x7f800000u);
  switch (mode) {
    case PF_GT_U4K:
      d = __fdiv_rn(a, x);
      e = x;
      break;
    case PF_GT_MID:
      d = __fdiv_rn(__fdiv_rn(a, x + b), 1000.0f);
      if (x == inf) d = 0.f;
      e = x == inf ? 0.f : x;
      break;
    case PF_GT_ETH3D:
      d = e = finite_or_zero(x);
      break;
    case PF_GT_GTA:
      d = e = __fdiv_rn(x, 256.0f);
      break;
    case PF_GT_CITYSCAPES:
      d = e = finite_or_zero(__fdiv_rn(a, x > 0.f ? __fdiv_rn(x - 1.0f, 256.0f) : x));
      break;
    default:                                                  // PF_GT_RAW
      d = e = x;
  }
}

template <int KIND, bool VEC>
__global__ __launch_bounds__(256) void gt_convert_kernel(const typename Sample<KIND>::raw* __restrict__ src, int H, int W, int mode, int swap,
                                                         int flip, float a, float b, float* __restrict__ depth, float* __restrict__ edge) {
  typedef typename Sample<KIND>::raw R;
  const int n = H * W;                                        // < 2^31 (checked by the caller): 32-bit indices inside the plane
  const int groups = (n + 3) >> 2;
  for (long gl = (long)blockIdx.x * blockDim.x + threadIdx.x; gl < groups; gl += (long)gridDim.x * blockDim.x) {
    const int i0 = (int)gl << 2;
    const int cnt = n - i0 < 4 ? n - i0 : 4;
    int y = 0, x = i0;
    if (flip) {
      y = i0 / W;
      x = i0 - y * W;
    }
    R r[4];
    if (VEC && cnt == 4) {                                    // four samples of one source row, aligned: W % 4 == 0 when flipped
      const int s0 = flip ? (H - 1 - y) * W + x : i0;
      const Raw4<R> q = *reinterpret_cast<const Raw4<R>*>(src + s0);
#pragma unroll
      for (int j = 0; j < 4; ++j) r[j] = q.v[j];
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        r[j] = 0;
        if (j < cnt) r[j] = src[flip ? (H - 1 - y) * W + x : i0 + j];
        if (flip && ++x == W) {
          x = 0;
          ++y;
        }
      }
    }
    float d[4], e[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) convert(mode, Sample<KIND>::get(r[j], swap != 0), a, b, d[j], e[j]);
    if (cnt == 4) {
      *reinterpret_cast<float4*>(depth + i0) = make_float4(d[0], d[1], d[2], d[3]);
      if (edge) *reinterpret_cast<float4*>(edge + i0) = make_float4(e[0], e[1], e[2], e[3]);
    } else {
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        if (j < cnt) {
          depth[i0 + j] = d[j];
          if (edge) edge[i0 + j] = e[j];
        }
      }
    }
  }
}

template <int KIND>
int launch(const void* src, int H, int W, int mode, int swap, int flip, float a, float b, float* depth, float* edge, hipStream_t stream) {
  typedef typename Sample<KIND>::raw R;
  if (reinterpret_cast<uintptr_t>(src) % sizeof(R)) return PF_ERR_ARG;
  const R* s = static_cast<const R*>(src);
  const int grid = grid_for(((long)H * W + 3) / 4, 256);
  const bool vec = reinterpret_cast<uintptr_t>(src) % 16 == 0 && (!flip || W % 4 == 0);
  if (vec)
    hipLaunchKernelGGL((gt_convert_kernel<KIND, true>), dim3(grid), dim3(256), 0, stream, s, H, W, mode, swap, flip, a, b, depth, edge);
  else
    hipLaunchKernelGGL((gt_convert_kernel<KIND, false>), dim3(grid), dim3(256), 0, stream, s, H, W, mode, swap, flip, a, b, depth, edge);
  return ok();
}

}  // namespace

extern "C" int pf_gt_convert(const void* src, int kind, int flags, int mode, int H, int W, float a, float b, float* depth, float* edge_src,
                             void* stream) {
  if (!src || !depth || H <= 0 || W <= 0) return PF_ERR_ARG;
  if ((long)H * W > 0x7fffffffL) return PF_ERR_ARG;                   // 32-bit indices inside the plane
  if (flags & ~(PF_GT_SWAP | PF_GT_FLIP)) return PF_ERR_ARG;
  if ((reinterpret_cast<uintptr_t>(depth) | reinterpret_cast<uintptr_t>(edge_src)) & 15u) return PF_ERR_ARG;   // 16-byte stores
  const bool is_float = kind == PF_GT_F16 || kind == PF_GT_F32 || kind == PF_GT_F64;
  const bool is_int = kind == PF_GT_U8 || kind == PF_GT_U16;
  const int swap = flags & PF_GT_SWAP ? 1 : 0, flip = flags & PF_GT_FLIP ? 1 : 0;
  bool pair;
  switch (mode) {                                                     // the table of include/pf_hip.h
    case PF_GT_U4K:
    case PF_GT_RAW: pair = is_float; break;
    case PF_GT_MID: pair = kind == PF_GT_F32; break;
    case PF_GT_ETH3D: pair = kind == PF_GT_F32 && !swap; break;
    case PF_GT_GTA:
    case PF_GT_CITYSCAPES: pair = is_int && !swap; break;
    default: return PF_ERR_ARG;
  }
  if (!pair) return PF_ERR_ARG;
  switch (kind) {
    case PF_GT_F16: return launch<PF_GT_F16>(src, H, W, mode, swap, flip, a, b, depth, edge_src, ST(stream));
    case PF_GT_F32: return launch<PF_GT_F32>(src, H, W, mode, swap, flip, a, b, depth, edge_src, ST(stream));
    case PF_GT_F64: return launch<PF_GT_F64>(src, H, W, mode, swap, flip, a, b, depth, edge_src, ST(stream));
    case PF_GT_U8: return launch<PF_GT_U8>(src, H, W, mode, swap, flip, a, b, depth, edge_src, ST(stream));
    default: return launch<PF_GT_U16>(src, H, W, mode, swap, flip, a, b, depth, edge_src, ST(stream));
  }
}
