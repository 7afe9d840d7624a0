// Backward kernels of the metric-bins head (engine.BinsHead) and of the SILog loss, float32, NHWC like the forward (csrc/imageops.hip,
// csrc/io.hip).  Formulas restated without autograd in tests/head_bwd_ref.py and held against float64 autograd through oracle/pf_oracle.py.
//
// No kernel here uses a float atomic: every sum has one fixed order (a serial loop, an MFMA chain, a butterfly over the lanes of one wave, or
// a second launch that adds partial results in index order), so two runs on the same operands give the same bits.
#include "pf_common.h"
#include "../../include/pf_hip.h"

namespace {

inline int grid_for(long n, int block) {
  long g = (n + block - 1) / block;
  return (int)(g > 16384 ? 16384 : (g < 1 ? 1 : g));
}
inline int ok() { return hipGetLastError() == hipSuccess ? PF_OK : PF_ERR_LAUNCH; }
#define ST(s) reinterpret_cast<hipStream_t>(s)
inline bool misaligned(const void* p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; }

// align_corners=True coordinates, the forward's own expression (csrc/imageops.hip ac_coord): the adjoint uses the weights the forward used
struct Lerp {
  int i0, i1;
  float l0, l1;
};
__device__ __forceinline__ Lerp ac_coord(int dst, float scale, int in) {
#pragma clang fp contract(off)
  const float src = scale * dst;
  Lerp r;
  r.i0 = (int)src;
  r.i1 = r.i0 + (r.i0 < in - 1 ? 1 : 0);
  r.l1 = src - r.i0;
  r.l0 = 1.0f - r.l1;
  return r;
}
inline float ac_scale(int in, int out) { return out > 1 ? (float)(in - 1) / (float)(out - 1) : 0.f; }
// weight of source index s in destination coordinate l (both taps may fall on s when the source axis has one element)
__device__ __forceinline__ float tap_weight(const Lerp& l, int s) { return (l.i0 == s ? l.l0 : 0.f) + (l.i1 == s ? l.l1 : 0.f); }
// destination range [lo, hi] that can touch source index s: scale * d in (s - 1, s + 1), widened by one either side and filtered by tap_weight
__device__ __forceinline__ void dst_range(int s, float scale, int out, int& lo, int& hi) {
  if (scale <= 0.f) { lo = 0; hi = out - 1; return; }
  const float inv = 1.0f / scale;
  lo = (int)floorf((float)(s - 1) * inv) - 1;
  hi = (int)ceilf((float)(s + 1) * inv) + 1;
  lo = lo < 0 ? 0 : lo;
  hi = hi > out - 1 ? out - 1 : hi;
}

// ------------------------------------------------------------------------------------------------
// weight gradient of a 1x1 layer: dW[n][k] = sum_p dY[p][n] X[p][k], db[n] = sum_p dY[p][n]
// ------------------------------------------------------------------------------------------------
// One block = one 64 (n) x 64 (k) tile of dW over `rpb` pixels: 32 pixels of both operands are staged in LDS per step (rows padded to 80
// floats: the four pixel rows that one v_mfma_f32_16x16x4_f32 operand load touches start 16 banks apart), wave w owns the 16 n-rows
// [16 w, 16 w + 16) and four 16 x 16 accumulators along k.  Operand map of the 16x16x4 float MFMA: lane l holds A[i = l & 15][kk = l >> 4] and
// B[kk = l >> 4][j = l & 15]; here i = n, j = k and kk walks the pixels, so both operands are read as LDS[pixel][channel] with the lane's low
// four bits on the channel.  C/D: column j = l & 15, row i = 4 (l >> 4) + reg.  Pixels past the block's range and channels past N / K are
// staged as zeros.  The bias gradient is the column sum of the staged dY tile, taken by the blocks of the first k-tile.
constexpr int WG_TILE = 64, WG_PIX = 32, WG_LD = 80;

__global__ __launch_bounds__(256) void wgrad_partial_kernel(const float* __restrict__ dy, int dy_ld, const float* __restrict__ x, int x_ld,
                                                            long P, int N, int K, int rpb, float* __restrict__ ws_w, float* __restrict__ ws_b) {
  __shared__ float sdy[WG_PIX][WG_LD], sx[WG_PIX][WG_LD];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, li = lane & 15, lk = lane >> 4;
  const int split = blockIdx.x, n0 = blockIdx.y * WG_TILE, k0 = blockIdx.z * WG_TILE;
  const long p_begin = (long)split * rpb;
  const long p_end = p_begin + rpb < P ? p_begin + rpb : P;
  const bool wave_on = n0 + 16 * wave < N;                         // wave-uniform: this wave's 16 n-rows exist
  const int nfrag = (K - k0 + 15) / 16 < 4 ? (K - k0 + 15) / 16 : 4;
  const bool do_bias = blockIdx.z == 0 && tid < WG_TILE;
  f32x4 acc[4];
#pragma unroll
  for (int f = 0; f < 4; ++f) acc[f] = f32x4{0.f, 0.f, 0.f, 0.f};
  float bsum = 0.f;
  const int col = tid & 63, row0 = tid >> 6;
  const bool n_ok = n0 + col < N, k_ok = k0 + col < K;
  for (long p = p_begin; p < p_end; p += WG_PIX) {
#pragma unroll
    for (int j = 0; j < WG_PIX / 4; ++j) {
      const int row = row0 + 4 * j;
      const long pp = p + row;
      const bool in = pp < p_end;
      sdy[row][col] = in && n_ok ? dy[pp * dy_ld + n0 + col] : 0.f;
      sx[row][col] = in && k_ok ? x[pp * x_ld + k0 + col] : 0.f;
    }
    __syncthreads();
    if (wave_on) {
#pragma unroll
      for (int s = 0; s < WG_PIX / 4; ++s) {
        const int r = 4 * s + lk;
        const float a = sdy[r][16 * wave + li];
#pragma unroll
        for (int f = 0; f < 4; ++f)
          if (f < nfrag) acc[f] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, sx[r][16 * f + li], acc[f], 0, 0, 0);
      }
    }
    if (do_bias) {
#pragma unroll 8
      for (int r = 0; r < WG_PIX; ++r) bsum += sdy[r][tid];
    }
    __syncthreads();
  }
  if (wave_on) {
    float* out = ws_w + (long)split * N * K;
#pragma unroll
    for (int f = 0; f < 4; ++f) {
      const int k = k0 + 16 * f + li;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int n = n0 + 16 * wave + 4 * lk + e;
        if (n < N && k < K) out[(long)n * K + k] = acc[f][e];
      }
    }
  }
  if (do_bias && n0 + tid < N) ws_b[(long)split * N + n0 + tid] = bsum;
}

// dW / db = the partial tiles added in split order
__global__ void wgrad_reduce_kernel(const float* __restrict__ ws_w, const float* __restrict__ ws_b, int splits, int N, int K,
                                    float* __restrict__ dw, float* __restrict__ db) {
  const long nk = (long)N * K, total = nk + (db ? N : 0);
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const bool is_w = i < nk;
    const float* src = is_w ? ws_w + i : ws_b + (i - nk);
    const long stride = is_w ? nk : N;
    float s = 0.f;
    for (int k = 0; k < splits; ++k) s += src[k * stride];
    if (is_w) dw[i] = s;
    else db[i - nk] = s;
  }
}

inline int wgrad_rows(long P, int rows_per_block) {
  if (rows_per_block > 0) return rows_per_block;
  long r = (P + 511) / 512;                                       // about 512 partials at the largest maps, never chains shorter than 512 pixels
  r = r < 512 ? 512 : r;
  return (int)((r + WG_PIX - 1) / WG_PIX * WG_PIX);
}

// ------------------------------------------------------------------------------------------------
// adjoint of the align_corners=True bilinear resize, as a gather: one thread per source element
// ------------------------------------------------------------------------------------------------
__global__ void resize_bwd_kernel(const float* __restrict__ dy, int dy_ld, int B, int OH, int OW, int C, float* __restrict__ dx, int dx_ld,
                                  int H, int W, int accumulate, float sh, float sw) {
  const long total = (long)B * H * W * C;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int c = (int)(i % C);
    const long pix = i / C;
    const int sx = (int)(pix % W), sy = (int)((pix / W) % H), b = (int)(pix / ((long)W * H));
    int y_lo, y_hi, x_lo, x_hi;
    dst_range(sy, sh, OH, y_lo, y_hi);
    dst_range(sx, sw, OW, x_lo, x_hi);
    float s = 0.f;
    for (int oy = y_lo; oy <= y_hi; ++oy) {
      const float wy = tap_weight(ac_coord(oy, sh, H), sy);
      if (wy == 0.f) continue;
      const float* row = dy + ((long)b * OH + oy) * OW * dy_ld + c;
      float r = 0.f;
      for (int ox = x_lo; ox <= x_hi; ++ox) {
        const float wx = tap_weight(ac_coord(ox, sw, W), sx);
        if (wx != 0.f) r += wx * row[(long)ox * dy_ld];
      }
      s += wy * r;
    }
    float* o = dx + pix * dx_ld + c;
    *o = accumulate ? *o + s : s;
  }
}

// ------------------------------------------------------------------------------------------------
// AttractorLayerUnnormed backward: one wave per pixel, lanes over the bins
//   c_j = up(b_prev)_j, dx = A_i - c_j, b_new_j = c_j + s sum_i f(dx)   ->   dA_i = s sum_j g_j f'(dx),  dc_j = g_j (1 - s sum_i f'(dx))
// ------------------------------------------------------------------------------------------------
template <bool EXP>
__device__ __forceinline__ float attractor_dfdx(float dx) {
  const float q = 300.0f * (dx * dx);
  if (EXP) return expf(-q) * (1.0f - 2.0f * q);
  const float d = 1.0f + q;
  return (1.0f - q) / (d * d);
}

template <bool EXP>
__global__ __launch_bounds__(256) void attractor_bwd_kernel(const float* __restrict__ A, int a_ld, int n_attr, float scale,
                                                            const float* __restrict__ bp, int hp, int wp, const float* __restrict__ g,
                                                            float* __restrict__ dA, int da_ld, float* __restrict__ dBc, int B, int h, int w,
                                                            int n_bins, float sh, float sw) {
  const int lane = threadIdx.x & 63;
  const long wave = ((long)blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = ((long)gridDim.x * blockDim.x) >> 6;
  const long npix = (long)B * h * w;
  for (long pix = wave; pix < npix; pix += nwaves) {
    const int ox = (int)(pix % w), oy = (int)((pix / w) % h), b = (int)(pix / ((long)w * h));
    const Lerp ly = ac_coord(oy, sh, hp), lx = ac_coord(ox, sw, wp);
    const long base = (long)b * hp * wp;
    const float* b00 = bp + (base + (long)ly.i0 * wp + lx.i0) * n_bins;
    const float* b01 = bp + (base + (long)ly.i0 * wp + lx.i1) * n_bins;
    const float* b10 = bp + (base + (long)ly.i1 * wp + lx.i0) * n_bins;
    const float* b11 = bp + (base + (long)ly.i1 * wp + lx.i1) * n_bins;
    float c[4], gj[4], fs[4];                                      // n_bins <= 256: at most four bins per lane
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      const int j = lane + 64 * m;
      const bool on = j < n_bins;
      c[m] = on ? ly.l0 * (lx.l0 * b00[j] + lx.l1 * b01[j]) + ly.l1 * (lx.l0 * b10[j] + lx.l1 * b11[j]) : 0.f;
      gj[m] = on ? g[pix * n_bins + j] : 0.f;
      fs[m] = 0.f;
    }
    const float* a = A + pix * a_ld;
    for (int i = 0; i < n_attr; ++i) {
      const float ai = a[i];
      float part = 0.f;
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        const float d = attractor_dfdx<EXP>(ai - c[m]);
        fs[m] += d;
        part += gj[m] * d;                                         // (gj is zero on the lanes past n_bins)
      }
      part = wave_sum(part);
      if (lane == 0) dA[pix * da_ld + i] = scale * part;
    }
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      const int j = lane + 64 * m;
      if (j < n_bins) dBc[pix * n_bins + j] = gj[m] * (1.0f - scale * fs[m]);
    }
  }
}

// ------------------------------------------------------------------------------------------------
// log-binomial expectation backward: one wave per pixel, lanes over the bins; the softmax is recomputed as in the forward
// ------------------------------------------------------------------------------------------------
// log C(n, k) in the Stirling form and y_k, every operation rounded on its own (no contraction) in torch's order: the float64 truth of the tests
// carries these float32 constants too (the oracle builds k and n as float32 tensors), and y / t amplifies a last-bit difference in log C --
// up to 3e-5 at values near 260 -- to 5e-6 of the gradient
__device__ __forceinline__ float logbinom_logc(float k, float n_, float eps) {
#pragma clang fp contract(off)
  const float k_ = k + eps;
  const float a = n_ * logf(n_), b = k_ * logf(k_), c = (n_ - k_) * logf(n_ - k_ + eps);
  return a - b - c;
}
__device__ __forceinline__ float logbinom_y(float logc, float k, float lp, float nk, float lq) {
#pragma clang fp contract(off)
  const float a = k * lp, b = nk * lq;
  return logc + a + b;
}

__global__ __launch_bounds__(256) void logbinom_bwd_kernel(const float* __restrict__ pt, int pt_ld, const float* __restrict__ cen, int hc, int wc,
                                                           const float* __restrict__ dd, float* __restrict__ dpt, int dpt_ld,
                                                           float* __restrict__ dcup, int B, int h, int w, int n_bins, float min_temp,
                                                           float max_temp, float sh, float sw, const float* __restrict__ logc_tab) {
  const float eps = 1e-7f;
  const float n_ = (float)(n_bins - 1) + eps;
  const int lane = threadIdx.x & 63;
  float logc[4];
#pragma unroll
  for (int m = 0; m < 4; ++m)      // the caller's table (the reference's own float32 constants) or the same expression evaluated here
    logc[m] = lane + 64 * m >= n_bins ? 0.f : logc_tab ? logc_tab[lane + 64 * m] : logbinom_logc((float)(lane + 64 * m), n_, eps);
  const long wave = ((long)blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = ((long)gridDim.x * blockDim.x) >> 6;
  const long npix = (long)B * h * w;
  for (long pix = wave; pix < npix; pix += nwaves) {
    const int ox = (int)(pix % w), oy = (int)((pix / w) % h), b = (int)(pix / ((long)w * h));
    const float* q = pt + pix * pt_ld;
    const float p0 = q[0] + 1e-4f, p1 = q[1] + 1e-4f, t0 = q[2] + 1e-4f, t1 = q[3] + 1e-4f;
    const float prob = p0 / (p0 + p1), tt = t0 / (t0 + t1);
    const float t = (max_temp - min_temp) * tt + min_temp;
    const float om_raw = 1.0f - prob;
    const float om = fminf(fmaxf(om_raw, 1e-4f), 1.0f), xc = fminf(fmaxf(prob, 1e-4f), 1.0f);
    const float lp = logf(xc), lq = logf(om);
    const Lerp ly = ac_coord(oy, sh, hc), lx = ac_coord(ox, sw, wc);
    const long base = (long)b * hc * wc;
    const float* c00 = cen + (base + (long)ly.i0 * wc + lx.i0) * n_bins;
    const float* c01 = cen + (base + (long)ly.i0 * wc + lx.i1) * n_bins;
    const float* c10 = cen + (base + (long)ly.i1 * wc + lx.i0) * n_bins;
    const float* c11 = cen + (base + (long)ly.i1 * wc + lx.i1) * n_bins;
    float y[4], c[4], pe[4];
    float mx = -INFINITY;
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      const int k = lane + 64 * m;
      const bool on = k < n_bins;
      y[m] = on ? logbinom_y(logc[m], (float)k, lp, (float)(n_bins - 1 - k), lq) : 0.f;
      c[m] = on ? ly.l0 * (lx.l0 * c00[k] + lx.l1 * c01[k]) + ly.l1 * (lx.l0 * c10[k] + lx.l1 * c11[k]) : 0.f;
      if (on) mx = fmaxf(mx, y[m] / t);
    }
    mx = wave_max(mx);
    // the bin of the largest probability (ties: the highest bin), its centre and its log C.  Everything below is taken relative to that bin:
    //   y_k - y_r = (logc_k - logc_r) + (k - k_r) (log x - log(1 - x))      (the (n - 1 - k) terms differ by -(k - k_r))
    // has the size of the difference, not of y (hundreds), so the exponent (y_k - y_r) / t is rounded at the scale that matters near the
    // peak, and the sums that cancel (sum_k dz_k = 0) round at the spread of the centres / of y under the softmax, not at their size
    float kr = -1.f;
#pragma unroll
    for (int m = 0; m < 4; ++m)
      if (lane + 64 * m < n_bins && y[m] / t == mx) kr = (float)(lane + 64 * m);
    kr = wave_max(kr);
    float cr = -INFINITY, lcr = -INFINITY;
#pragma unroll
    for (int m = 0; m < 4; ++m)
      if ((float)(lane + 64 * m) == kr) { cr = c[m]; lcr = logc[m]; }
    cr = wave_max(cr);
    lcr = wave_max(lcr);
    const float dl = lp - lq;
    float num = 0.f, den = 0.f;
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      const bool on = lane + 64 * m < n_bins;
      y[m] = on ? (logc[m] - lcr) + ((float)(lane + 64 * m) - kr) * dl : 0.f;      // y_k - y_r from here on
      pe[m] = on ? expf(y[m] / t) : 0.f;
      c[m] -= cr;
      num += pe[m] * c[m];
      den += pe[m];
    }
    num = wave_sum(num);
    den = wave_sum(den);
    const float depth = num / den, gd = dd[pix];                 // depth - cr
    // dz_k = probs_k (c_k - depth) g;  y_k = logc_k + k log x + (n - 1 - k) log(1 - x),  z_k = y_k / t;  sum_k dz_k (n - 1 - k) = -sum_k dz_k k
    float s_k = 0.f, s_y = 0.f;
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      const int k = lane + 64 * m;
      if (k < n_bins) {
        const float pr = pe[m] / den;
        dcup[pix * n_bins + k] = pr * gd;
        const float dz = pr * (c[m] - depth) * gd;
        s_k += dz * ((float)k - kr);
        s_y += dz * y[m];
      }
    }
    s_k = wave_sum(s_k);
    s_y = wave_sum(s_y);
    const float s_nk = -s_k;
    if (lane == 0) {
      // the clamps pass the gradient where the value lies inside [1e-4, 1] (bounds included, as torch.clamp's backward does)
      float dprob = 0.f;
      if (prob >= 1e-4f && prob <= 1.0f) dprob += (s_k / t) / xc;
      if (om_raw >= 1e-4f && om_raw <= 1.0f) dprob -= (s_nk / t) / om;
      const float dtt = -(s_y / (t * t)) * (max_temp - min_temp);
      const float ps = (p0 + p1) * (p0 + p1), ts = (t0 + t1) * (t0 + t1);
      float* o = dpt + pix * dpt_ld;
      o[0] = dprob * p1 / ps;
      o[1] = -dprob * p0 / ps;
      o[2] = dtt * t1 / ts;
      o[3] = -dtt * t0 / ts;
    }
  }
}

// ------------------------------------------------------------------------------------------------
// dy *= act'(.)   relu / softplus from the layer's output, gelu (exact erf form) from the pre-activation
// ------------------------------------------------------------------------------------------------
__global__ void act_bwd_kernel(float* __restrict__ dy, int dy_ld, const float* __restrict__ ref, int ref_ld, long P, int C, int act) {
  const long total = P * C;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int c = (int)(i % C);
    const long p = i / C;
    const float v = ref[p * ref_ld + c];
    float d;
    if (act == PF_ACT_RELU) d = v > 0.f ? 1.f : 0.f;
    else if (act == PF_ACT_SOFTPLUS) d = -expm1f(-v);            // y = log(1 + e^x)  ->  sigmoid(x) = 1 - e^-y, without the cancellation at small y (1 in float32 past the threshold of 20)
    else d = 0.5f * (1.0f + erff(v * 0.70710678118654752440f)) + v * 0.3989422804014327f * expf(-0.5f * v * v);
    dy[p * dy_ld + c] *= d;
  }
}

// ------------------------------------------------------------------------------------------------
// SILog loss backward from the forward's saved sums s = (n, sum g, sum g^2):
//   L = 10 sqrt(V + beta m^2), m = s1 / n, V = (s2 - s1^2 / n) / (n - 1)  ->  dL/dg_i = (10 / R) ((g_i - m) / (n - 1) + beta m / n), R = L / 10
// ------------------------------------------------------------------------------------------------
__global__ void silog_bwd_kernel(const float* __restrict__ pred, const float* __restrict__ target, long n, float lo, float hi, float beta,
                                 const double* __restrict__ s, float dloss, float* __restrict__ dpred) {
  const double cnt = s[0];
  const bool live = cnt > 1.0;
  const double mean = live ? s[1] / cnt : 0.0;
  const double var = live ? fmax((s[2] - s[1] * s[1] / cnt) / (cnt - 1.0), 0.0) : 0.0;
  const double R = sqrt(var + (double)beta * mean * mean);
  const double k0 = live && R > 0.0 ? 10.0 * (double)dloss / R : 0.0;
  const double kv = k0 / (cnt - 1.0), km = k0 * (double)beta * mean / cnt;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const float t = target[i];
    float d = 0.f;
    if (live && t > lo && t < hi) {
      const float pe = pred[i] + 1e-7f;
      const float g = logf(pe) - logf(t + 1e-7f);
      d = (float)((((double)g - mean) * kv + km) / (double)pe);
    }
    dpred[i] = d;
  }
}

}  // namespace

extern "C" int pf_conv1x1_wgrad_workspace_bytes(long P, int N, int K, int rows_per_block, long* bytes) {
  if (!bytes || P < 1 || N < 1 || K < 1 || N > 4096 || K > 4096 || rows_per_block < 0) return PF_ERR_ARG;
  const int rpb = wgrad_rows(P, rows_per_block);
  const long splits = (P + rpb - 1) / rpb;
  if (splits > 65535) return PF_ERR_ARG;
  *bytes = splits * ((long)N * K + N) * 4;
  return PF_OK;
}

extern "C" int pf_conv1x1_wgrad(const float* dy, int dy_ld, const float* x, int x_ld, long P, int N, int K, float* dw, float* db,
                                void* workspace, long workspace_bytes, int rows_per_block, void* stream) {
  if (!dy || !x || !dw || !workspace) return PF_ERR_ARG;
  if (misaligned(dy, 4) || misaligned(x, 4) || misaligned(dw, 4) || misaligned(db, 4) || misaligned(workspace, 4)) return PF_ERR_ARG;
  if (dy_ld < N || x_ld < K) return PF_ERR_ARG;
  long need = 0;
  if (pf_conv1x1_wgrad_workspace_bytes(P, N, K, rows_per_block, &need) != PF_OK || workspace_bytes < need) return PF_ERR_ARG;
  const int rpb = wgrad_rows(P, rows_per_block);
  const int splits = (int)((P + rpb - 1) / rpb);
  const int nt = (N + WG_TILE - 1) / WG_TILE, kt = (K + WG_TILE - 1) / WG_TILE;
  float* ws_w = static_cast<float*>(workspace);
  float* ws_b = ws_w + (long)splits * N * K;
  hipLaunchKernelGGL(wgrad_partial_kernel, dim3(splits, nt, kt), dim3(256), 0, ST(stream), dy, dy_ld, x, x_ld, P, N, K, rpb, ws_w, ws_b);
  hipLaunchKernelGGL(wgrad_reduce_kernel, dim3(grid_for((long)N * K + N, 256)), dim3(256), 0, ST(stream), ws_w, ws_b, splits, N, K, dw, db);
  return ok();
}

extern "C" int pf_resize_bilinear_bwd(const float* dy, int dy_ld, int B, int OH, int OW, int C, float* dx, int dx_ld, int H, int W,
                                      int accumulate, void* stream) {
  if (!dy || !dx || misaligned(dy, 4) || misaligned(dx, 4)) return PF_ERR_ARG;
  if (B < 1 || OH < 1 || OW < 1 || H < 1 || W < 1 || C < 1 || dy_ld < C || dx_ld < C) return PF_ERR_ARG;
  const long total = (long)B * H * W * C;
  hipLaunchKernelGGL(resize_bwd_kernel, dim3(grid_for(total, 256)), dim3(256), 0, ST(stream), dy, dy_ld, B, OH, OW, C, dx, dx_ld, H, W,
                     accumulate, ac_scale(H, OH), ac_scale(W, OW));
  return ok();
}

extern "C" int pf_attractor_bwd(const float* A, int a_ld, int n_attr, int attractor_exp, int kind_sum, const float* b_prev, int hp, int wp,
                                const float* d_b_new, float* dA, int da_ld, float* d_b_c, int B, int h, int w, int n_bins, void* stream) {
  if (!A || !b_prev || !d_b_new || !dA || !d_b_c) return PF_ERR_ARG;
  if (misaligned(A, 4) || misaligned(b_prev, 4) || misaligned(d_b_new, 4) || misaligned(dA, 4) || misaligned(d_b_c, 4)) return PF_ERR_ARG;
  if (n_attr < 1 || a_ld < n_attr || da_ld < n_attr || n_bins < 1 || n_bins > 256 || B < 1 || h < 1 || w < 1 || hp < 1 || wp < 1) return PF_ERR_ARG;
  const long npix = (long)B * h * w;
  const float scale = kind_sum ? 1.0f : 1.0f / (float)n_attr;
  if (attractor_exp)
    hipLaunchKernelGGL(attractor_bwd_kernel<true>, dim3(grid_for(npix, 4)), dim3(256), 0, ST(stream), A, a_ld, n_attr, scale, b_prev, hp, wp,
                       d_b_new, dA, da_ld, d_b_c, B, h, w, n_bins, ac_scale(hp, h), ac_scale(wp, w));
  else
    hipLaunchKernelGGL(attractor_bwd_kernel<false>, dim3(grid_for(npix, 4)), dim3(256), 0, ST(stream), A, a_ld, n_attr, scale, b_prev, hp, wp,
                       d_b_new, dA, da_ld, d_b_c, B, h, w, n_bins, ac_scale(hp, h), ac_scale(wp, w));
  return ok();
}

extern "C" int pf_logbinom_depth_bwd(const float* pt, int pt_ld, const float* centers, int hc, int wc, const float* d_depth, float* d_pt,
                                     int d_pt_ld, float* d_centers_up, int B, int h, int w, int n_bins, float min_temp, float max_temp,
                                     const float* logc, void* stream) {
  if (!pt || !centers || !d_depth || !d_pt || !d_centers_up) return PF_ERR_ARG;
  if (misaligned(pt, 4) || misaligned(centers, 4) || misaligned(d_depth, 4) || misaligned(d_pt, 4) || misaligned(d_centers_up, 4) || misaligned(logc, 4)) return PF_ERR_ARG;
  if (pt_ld < 4 || d_pt_ld < 4 || n_bins < 2 || n_bins > 256 || B < 1 || h < 1 || w < 1 || hc < 1 || wc < 1) return PF_ERR_ARG;
  const long npix = (long)B * h * w;
  hipLaunchKernelGGL(logbinom_bwd_kernel, dim3(grid_for(npix, 4)), dim3(256), 0, ST(stream), pt, pt_ld, centers, hc, wc, d_depth, d_pt, d_pt_ld,
                     d_centers_up, B, h, w, n_bins, min_temp, max_temp, ac_scale(hc, h), ac_scale(wc, w), logc);
  return ok();
}

extern "C" int pf_act_bwd(float* dy, int dy_ld, const float* ref, int ref_ld, long P, int C, int act, void* stream) {
  if (!dy || !ref || misaligned(dy, 4) || misaligned(ref, 4)) return PF_ERR_ARG;
  if (P < 1 || C < 1 || dy_ld < C || ref_ld < C) return PF_ERR_ARG;
  if (act != PF_ACT_RELU && act != PF_ACT_GELU && act != PF_ACT_SOFTPLUS) return PF_ERR_ARG;
  hipLaunchKernelGGL(act_bwd_kernel, dim3(grid_for(P * C, 256)), dim3(256), 0, ST(stream), dy, dy_ld, ref, ref_ld, P, C, act);
  return ok();
}

extern "C" int pf_silog_loss_bwd(const float* pred, const float* target, long n, float min_depth, float max_depth, float beta,
                                 const double* sums3, float d_loss, float* d_pred, void* stream) {
  if (!pred || !target || !sums3 || !d_pred || n <= 0) return PF_ERR_ARG;
  if (misaligned(pred, 4) || misaligned(target, 4) || misaligned(sums3, 8) || misaligned(d_pred, 4)) return PF_ERR_ARG;
  hipLaunchKernelGGL(silog_bwd_kernel, dim3(grid_for(n, 256)), dim3(256), 0, ST(stream), pred, target, n, min_depth, max_depth, beta, sums3,
                     d_loss, d_pred);
  return ok();
}
