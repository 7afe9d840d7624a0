// MiDaS BEiT-L core (DPT_BEiT_L_384, the relative-depth core of a type-'ZoeDepth' branch) kernels other than the linear layers and the attention
// (those run on gemm_split3.hip / igemm.hip and attn_split3.hip pf_vit_attention_split3_rpb): the P x P patch im2col with per-channel mean / std
// (MiDaS PrepForMidas Normalize(0.5, 0.5), midas.py:160-169, + BEiT patch_embed.proj) and the readout-'project' operand rows [token | cls].
#include "pf_common.h"
#include "../../include/pf_hip.h"
#include "pf_args.h"

namespace {

struct Norm3 {
  float mean[3], stdv[3];
};

// out[(b,ty,tx)][(ky*P+kx)*3 + c] = (img[b,c,ty*P+ky,tx*P+kx] - mean[c]) / std[c], columns 3 P^2 .. ld-1 zero
__global__ void patch_im2col_norm_kernel(const float* __restrict__ img, int B, int H, int W, int P, Norm3 n, float* __restrict__ out, int ld) {
  const int th = H / P, tw = W / P, K = 3 * P * P;
  const long total = (long)B * th * tw * ld;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int k = (int)(i % ld);
    const long row = i / ld;
    float v = 0.f;
    if (k < K) {
      const int c = k % 3, kk = k / 3, kx = kk % P, ky = kk / P;
      const int tx = (int)(row % tw), ty = (int)((row / tw) % th), b = (int)(row / ((long)tw * th));
      const float px = img[(((long)b * 3 + c) * H + (ty * P + ky)) * W + (tx * P + kx)];
      v = (px - n.mean[c]) / n.stdv[c];
    }
    out[i] = v;
  }
}

// y[b*T + t][0:D] = x[b*S + 1 + t][0:D], y[b*T + t][D:2D] = x[b*S][0:D]  (T = S - 1; float4 granules, D % 4 == 0)
__global__ void readout_concat_kernel(const float* __restrict__ x, int x_ld, int B, int S, int D, float* __restrict__ y, int y_ld) {
  const int D4 = D / 4, T = S - 1;
  const long total = (long)B * T * 2 * D4;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int c = (int)(i % (2 * D4));
    const long row = i / (2 * D4);
    const int b = (int)(row / T), t = (int)(row - (long)b * T);
    const long src = c < D4 ? (long)b * S + 1 + t : (long)b * S;
    const int col = (c < D4 ? c : c - D4) * 4;
    *reinterpret_cast<float4*>(y + row * y_ld + 4 * c) = *reinterpret_cast<const float4*>(x + src * x_ld + col);
  }
}

inline int grid_for(long n, int block) {
  long g = (n + block - 1) / block;
  return (int)(g < 8192 ? (g > 0 ? g : 1) : 8192);
}

}  // namespace

extern "C" int pf_patch_im2col_norm(const float* img, int B, int H, int W, int patch, const float* mean3, const float* std3, float* out, int ld,
                                    void* stream) {
  if (!img || !out || !mean3 || !std3) return pf_refuse("pf_patch_im2col_norm", "null pointer");
  if (pf_misaligned(img, 4) || pf_misaligned(out, 4) || pf_misaligned(mean3, 4) || pf_misaligned(std3, 4)) return pf_refuse("pf_patch_im2col_norm", "misaligned pointer");
  if (B <= 0 || H <= 0 || W <= 0 || patch <= 0 || patch > 1024 || H % patch || W % patch || ld < 3 * patch * patch)
    return pf_refuse("pf_patch_im2col_norm", "B, H, W must be positive, H and W multiples of patch <= 1024, ld >= 3 patch^2");
  Norm3 n;
  for (int c = 0; c < 3; ++c) {
    if (!(std3[c] != 0.f) || std3[c] != std3[c]) return pf_refuse("pf_patch_im2col_norm", "std must not be zero (or NaN)");
    n.mean[c] = mean3[c];
    n.stdv[c] = std3[c];
  }
  const long total = (long)B * (H / patch) * (W / patch) * ld;
  hipLaunchKernelGGL(patch_im2col_norm_kernel, dim3(grid_for(total, 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), img, B, H, W, patch, n, out,
                     ld);
  return hipGetLastError() == hipSuccess ? PF_OK : PF_ERR_LAUNCH;
}

extern "C" int pf_readout_concat(const float* x, int x_ld, int B, int S, int D, float* y, int y_ld, void* stream) {
  if (!x || !y) return pf_refuse("pf_readout_concat", "null tensor");
  if (B <= 0 || S < 2 || D <= 0 || D % 4 || x_ld % 4 || y_ld % 4 || x_ld < D || y_ld < 2L * D)
    return pf_refuse("pf_readout_concat", "B >= 1, S >= 2, D, x_ld, y_ld multiples of 4, x_ld >= D, y_ld >= 2 D");
  if (pf_misaligned(x, 16) || pf_misaligned(y, 16)) return pf_refuse("pf_readout_concat", "misaligned tensor");
  const long total = (long)B * (S - 1) * (D / 2);
  hipLaunchKernelGGL(readout_concat_kernel, dim3(grid_for(total, 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), x, x_ld, B, S, D, y, y_ld);
  return hipGetLastError() == hipSuccess ? PF_OK : PF_ERR_LAUNCH;
}
