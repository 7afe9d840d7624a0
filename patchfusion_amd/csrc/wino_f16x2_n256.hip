// fp16x2 transform-domain GEMM on 128 x 128 tiles: the three-step Winograd layers whose whole-layer product routes to PF_S3_ROUTE_PERSIST128 (the
// 256-column layers of the DPT head: layer_rn, the RCUs, the fusion net's double convs).  Operands and arithmetic are those of the 192-tile form
// (csrc/wino_f16x2.hip header, csrc/gemm_split3.hip F16): V / 2^e_c and U' / 2^f_pn as two chunk-major fp16 planes each, three products per
// accumulator (w_h.x_l, w_l.x_h, w_h.x_h, smallest first) on v_mfma_f32_16x16x32_f16, M = ldexp(acc, f_pn).  Same K-chunk order and the same
// three terms per accumulator as the 192-tile kernel, so an output element does not depend on which tile computed it.
//
// Walk, loader, ring and phases are those of gemm_split3_persist_kernel (csrc/gemm_split3.hip, "PERSISTENT ping-pong form"): one resident block of
// eight waves per CU walks its share of the tiles, channel tile fastest; the K chunks of consecutive tiles form one stream through a THREE-slot ring;
// group A (waves 0-3, stages the V planes) and group B (waves 4-7, the U' planes) alternate load and multiply phases, B one phase behind.
// A stage is 2 planes x (128 + 128) rows x 64 B = 32 KiB (bf16x3: 48 KiB), the ring 96 KiB; a wave moves PPW = 4 LDS-DMA pieces per chunk
// (bf16x3: 6), reads 12 fragments (18) and issues 24 MFMAs (48).
// Hand-counted waits, over LDS-DMA pieces only: vmcnt(4) = this wave's four pieces of the newest chunk may still fly, everything older has landed;
// vmcnt(0) at the ring's fill (fewer than three chunks) and at the stream's end.  The epilogue's exponent loads and its stores are issued at the head
// of a load phase, BEFORE that phase's pieces: they are older than the four pieces a counted wait lets fly, so however they retire relative to DMA
// pieces they cannot make a count pass early (never count register loads in a hand-counted wait).
// Epilogue on exchanged fragments, as in the 192-tile kernel: lanes fr < 8 trade their fn+1 fragment for the fn fragment of lane fr + 8 (DPP
// row_ror:8), so that every 16-byte store of a lane pair completes 128-byte lines (DESIGN.md 0 names the tile-switch store burst as what holds the
// bf16x3 128-tile kernel down at K = 256; whether this epilogue removes it was not measured).
// The file also holds wino_output_cmax_kernel: the output transform that hands the channel maxima of its output to a following fp16x2 layer.
#include <atomic>
#include <cstdlib>
#include "pf_common.h"
#include "../../include/pf_hip.h"
#include "pf_args.h"
#include "pf_launch.h"

namespace {

__device__ __forceinline__ unsigned lds_addr(const void* p) {
  return (unsigned)(size_t)(__attribute__((address_space(3))) const char*)p;
}
// one LDS-DMA piece: 64 lanes x 16 bytes from a wave-uniform base + per-lane offset into 1 KiB of LDS at m0
__device__ __forceinline__ void glds16s(unsigned voff, unsigned long long sbase, unsigned lds_dst) {
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
               : "=&s"(keep)
               : "v"(voff), "s"(sbase), "s"(lds_dst)
               : "memory");
}
template <int N>
__device__ __forceinline__ void vm_wait() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }
// barrier that does not drain the DMA queue
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }
// barrier without waiting for this wave's own LDS reads
__device__ __forceinline__ void plain_barrier() {
  __builtin_amdgcn_sched_barrier(0);
  asm volatile("s_barrier" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);
}

// p.scale carries the int32 column exponents [batch][w_rows]; mt / nt = token / channel tiles per transform point, total = tiles of the launch
__global__ __launch_bounds__(512) void gemm_f16x2_persist128_kernel(const pf_conv_params p, int mt, int nt, int total) {
  constexpr int BM = 128, BN = 128, WM = 4, WN = 2, NP = 2, NS = 3;
  constexpr int NW = WM * WN;
  constexpr int WTM = BM / WM, WTN = BN / WN, FM = WTM / 16, FN = WTN / 16;
  constexpr int ROWS = NP * (BM + BN), PIECES = ROWS / 16, PPW = PIECES / NW;
  constexpr int STAGE = ROWS * 64;
  static_assert(PPW == 4 && PPW * 16 * WM == NP * BM && WM * 2 == NW && BM == BN && FN % 2 == 0, "waves 0..3 stage the V planes, waves 4..7 the U' planes");
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WN, wn = wave % WN;
  const int M = p.B * p.OH * p.OW;
  const int nk = p.Cin / 32;

  // ---- this block's tiles: XCD x owns the contiguous range [total x / 8, total (x+1) / 8); order = point > token tile > channel tile
  const int G = (int)gridDim.x, xcd = (int)blockIdx.x & 7, nb = (G - xcd + 7) >> 3;
  const int lo = (int)((long)total * xcd / 8), hi = (int)((long)total * (xcd + 1) / 8);
  const int l_first = lo + ((int)blockIdx.x >> 3);
  if (l_first >= hi) return;
  const int my_tiles = (hi - l_first + nb - 1) / nb;
  const int chunks = my_tiles * nk;
  const int per_plane = mt * nt;
  auto decode = [&](int l, int& z, int& m0, int& n0) __attribute__((always_inline)) {
    z = l / per_plane;
    const int r = l - z * per_plane;
    const int t = r / nt;
    m0 = t * BM;
    n0 = (r - t * nt) * BN;
  };

  // ---- loader: wave w moves pieces w*PPW .. +PPW-1 of a stage [V h | V l | U' h | U' l]; lane L -> row 16 q + (L >> 2), physical slot
  // L & 3 = logical slot ^ ((row >> 1) & 3).  Both operands are chunk-major: a row is 64 B, a K chunk of all rows one slab of lim x 64 B.
  // Rows beyond M / w_rows are clamped to the last valid row: their products land in accumulator rows / columns that are never stored.
  const bool is_x = wave < WM;
  const int lim = is_x ? M : p.w_rows;
  const unsigned adv_b = (unsigned)lim * 64u;
  const unsigned long long op_base = is_x ? (unsigned long long)p.x : (unsigned long long)p.w;
  const unsigned long long pl_b = (unsigned long long)(is_x ? p.x_bstride : p.w_bstride) * 2;   // h / l plane pitch in bytes
  const unsigned long long z_b = (unsigned long long)lim * (unsigned long long)(p.Cin * 2);      // transform-point pitch in bytes
  unsigned long long sbase[PPW];
  unsigned voff[PPW];
  auto setup_loader = [&](int l) __attribute__((always_inline)) {
    int z, m0, n0;
    decode(l, z, m0, n0);
    const int origin = is_x ? m0 : n0;
    const unsigned long long tb = op_base + (unsigned long long)z * z_b + (unsigned long long)origin * 64u;
    const int last = lim - 1 - origin;
#pragma unroll
    for (int i = 0; i < PPW; ++i) {
      const int pc = (wave & (WM - 1)) * PPW + i;                                // piece within this operand's two planes
      const int row = pc * 16 + (lane >> 2);
      const int j = (lane & 3) ^ ((row >> 1) & 3);                               // (BM is a multiple of 8: same swizzle as the stage row)
      const int pl = pc / (BM / 16), r = row - pl * BM;
      sbase[i] = tb + pl * pl_b;
      voff[i] = (unsigned)(min(r, last) * 64 + j * 16);
    }
  };
  const unsigned smem_base = lds_addr(smem);
  int l_load = l_first, l_kc = -1, s_issue = NS - 1;
  unsigned dst_cur = 0;
  setup_loader(l_load);
  auto issue = [&]() __attribute__((always_inline)) {    // a whole chunk from the load phase: ring slot, chunk within the tile, tile switch
    s_issue = s_issue == NS - 1 ? 0 : s_issue + 1;
    if (++l_kc == nk) {
      l_kc = 0;
      l_load += nb;
      if (l_load < hi) setup_loader(l_load);
    }
    dst_cur = __builtin_amdgcn_readfirstlane(smem_base + s_issue * STAGE + wave * (PPW * 1024));
#pragma unroll
    for (int i = 0; i < PPW; ++i) {
      glds16s(voff[i], sbase[i], dst_cur + i * 1024);
      sbase[i] += adv_b;
    }
  };

  f32x4 acc[FN][FM];
#pragma unroll
  for (int fn = 0; fn < FN; ++fn)
#pragma unroll
    for (int fm = 0; fm < FM; ++fm) acc[fn][fm] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int fr = lane & 15, fg = lane >> 4;
  const int slot = (fg ^ ((fr >> 1) & 3)) << 4;
  const int x_off = (wm * WTM + fr) * 64 + slot;
  const int w_off = NP * BM * 64 + (wn * WTN + fr) * 64 + slot;
  struct Frags { uint4 w[NP][FN], x[NP][FM]; };
  int s_read = 0;
  auto read_frags = [&](Frags& f) __attribute__((always_inline)) {
    const char* S = smem + s_read * STAGE;
    s_read = s_read == NS - 1 ? 0 : s_read + 1;
#pragma unroll
    for (int pl = 0; pl < NP; ++pl) {
#pragma unroll
      for (int fn = 0; fn < FN; ++fn) f.w[pl][fn] = *reinterpret_cast<const uint4*>(S + w_off + pl * (BN * 64) + fn * 1024);
#pragma unroll
      for (int fm = 0; fm < FM; ++fm) f.x[pl][fm] = *reinterpret_cast<const uint4*>(S + x_off + pl * (BM * 64) + fm * 1024);
    }
  };
#define F16_TERM(PW, PX)                                                                                                     \
  _Pragma("unroll") for (int fn = 0; fn < FN; ++fn) _Pragma("unroll") for (int fm = 0; fm < FM; ++fm)                       \
      acc[fn][fm] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, f.w[PW][fn]), __builtin_bit_cast(f16x8, f.x[PX][fm]), \
                                                           acc[fn][fm], 0, 0, 0);
  auto multiply = [&](const Frags& f) __attribute__((always_inline)) {
    F16_TERM(0, 1) F16_TERM(1, 0) F16_TERM(0, 0)
  };
#undef F16_TERM

  // ---- epilogue of the tile whose last chunk was just multiplied: coordinates decoded in that chunk's load phase, stores one phase later
  int l_comp = l_first, c_kc = 0;
  int e_z = 0, e_m0 = 0, e_n0 = 0;
  bool epi_pending = false;
  auto epilogue = [&]() __attribute__((always_inline)) {
    float* yb = reinterpret_cast<float*>(p.y) + (long)e_z * M * p.y_ld;
    const int* fx = reinterpret_cast<const int*>(p.scale) + (long)e_z * p.w_rows;
    const bool lo8 = fr < 8;
#pragma unroll
    for (int fn = 0; fn < FN; fn += 2) {
      const int n = e_n0 + wn * WTN + (fn + (lo8 ? 0 : 1)) * 16 + fg * 4;       // the fragment whose values this lane stores
      const bool nok = n < p.Cout;
      int4 fexp = make_int4(0, 0, 0, 0);
      if (nok) fexp = *reinterpret_cast<const int4*>(fx + n);
      const int fe[4] = {fexp.x, fexp.y, fexp.z, fexp.w};
#pragma unroll
      for (int fm = 0; fm < FM; ++fm) {
        const f32x4 a = acc[fn][fm], b = acc[fn + 1][fm];
        acc[fn][fm] = f32x4{0.f, 0.f, 0.f, 0.f};
        acc[fn + 1][fm] = f32x4{0.f, 0.f, 0.f, 0.f};
        float v[2][4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float snd = lo8 ? b[r] : a[r];
          const float recv = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, snd), 0x128, 0xf, 0xf, false));   // row_ror:8
          v[0][r] = ldexpf(lo8 ? a[r] : recv, fe[r]);
          v[1][r] = ldexpf(lo8 ? recv : b[r], fe[r]);
        }
        const int m1 = e_m0 + wm * WTM + fm * 16 + (fr & 7);
        if (nok && m1 < M) *reinterpret_cast<float4*>(yb + (long)m1 * p.y_ld + n) = make_float4(v[0][0], v[0][1], v[0][2], v[0][3]);
        if (nok && m1 + 8 < M) *reinterpret_cast<float4*>(yb + (long)(m1 + 8) * p.y_ld + n) = make_float4(v[1][0], v[1][1], v[1][2], v[1][3]);
      }
    }
    epi_pending = false;
  };

  // ---- the chunk stream: a second copy of gemm_split3_persist_kernel's control flow (schedule and hazards described there), to be kept in step with it.
  // Slot g % 3 is re-issued only after both groups read chunk g (lgkmcnt(0) + barrier); the early return above is before any barrier.
#pragma nounroll
  for (int i = 0; i < NS; ++i)
    if (i < chunks) issue();
  if (chunks > 2) vm_wait<PPW>();                       // chunks 0 and 1 landed
  else vm_wait<0>();
  lds_barrier();
  Frags fa, fb;
  read_frags(fa);
  lds_barrier();
  const bool grp_b = wave >= NW / 2;
  if (grp_b) plain_barrier();                           // one phase behind
  // phase M(g): [stores of the tile that ended with chunk g-1], DMA of chunk g+3, fragments of chunk g+1, wait for this wave's pieces of g+2;
  // phase C(g): the 24 MFMAs of chunk g out of registers
  auto pp_chunk = [&](const Frags& cf, Frags& nf, int g) __attribute__((always_inline)) {
    if (epi_pending) epilogue();                        // beside the partner group's MFMAs
    if (c_kc == nk - 1) {                               // chunk g ends a tile
      decode(l_comp, e_z, e_m0, e_n0);
      l_comp += nb;
    }
    if (g + 3 < chunks) issue();
    if (g + 1 < chunks) read_frags(nf);
    if (g + 3 < chunks) vm_wait<PPW>();
    else if (g + 2 < chunks) vm_wait<0>();
    lds_barrier();
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_setprio(1);
    multiply(cf);
    __builtin_amdgcn_s_setprio(0);
    if (++c_kc == nk) { c_kc = 0; epi_pending = true; }
    plain_barrier();
  };
#pragma nounroll
  for (int g = 0; g < chunks; g += 2) {
    pp_chunk(fa, fb, g);
    if (g + 1 < chunks) pp_chunk(fb, fa, g + 1);
  }
  if (!grp_b) plain_barrier();
  epilogue();
}


// ---- output transform that also hands the channel maxima of what it stores to the next layer (the range pass of an fp16x2 consumer, for nothing) ----
// A^T m A of F(4x4,3x3) along one axis (the same arithmetic as csrc/winograd.hip Wino<4>::at)
__device__ __forceinline__ void at6(const float (&m)[6], float (&o)[4]) {
  const float s12 = m[1] + m[2], d12 = m[1] - m[2], s34 = m[3] + m[4], d34 = m[3] - m[4];
  o[0] = m[0] + s12 + s34;
  o[1] = d12 + 2.f * d34;
  o[2] = s12 + 4.f * s34;
  o[3] = d12 + 8.f * d34 + m[5];
}

// wino_output_kernel<4> of csrc/winograd.hip, statement for statement (same bits in y), plus: cmax[c] = max over the stored pixels of |y| (cmax_relu:
// of max(y, 0), what a consumer with relu_in reads) as float bits -- registers -> the block's LDS copy -> one global atomicMax per channel and block,
// the scheme of wino_absmax_kernel: a uint max of non-negative float bits is order-free, so the result is bit-reproducible and equals the range pass's.
__global__ __launch_bounds__(512) void wino_output_cmax_kernel(const float* __restrict__ M, int N, const float* __restrict__ bias, int relu,
                                                               const float* __restrict__ res, int res_ld, const float* __restrict__ res2,
                                                               int res2_ld, float* __restrict__ y, int y_ld, int B, int H, int W, int TH,
                                                               int TW, long tile0, long T, unsigned* __restrict__ cmax, int cmax_relu) {
  constexpr int MT = 4, A = 6;
  extern __shared__ unsigned sm[];
  for (int i = threadIdx.x; i < N; i += blockDim.x) sm[i] = 0u;
  __syncthreads();
  const int nv = N >> 2;
  for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < T * nv; idx += (long)gridDim.x * blockDim.x) {
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
      at6(col[e], o);
#pragma unroll
      for (int p = 0; p < MT; ++p) t[p][j][e] = o[p];
    }
  }
  float4 bv = make_float4(0.f, 0.f, 0.f, 0.f);
  if (bias) bv = *reinterpret_cast<const float4*>(bias + n4 * 4);
  const float be[4] = {bv.x, bv.y, bv.z, bv.w};
  uint32_t mx[4] = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int p = 0; p < MT; ++p) {
    const int oy = ty * MT + p;
    float r[4][MT];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float row[A];
#pragma unroll
      for (int j = 0; j < A; ++j) row[j] = t[p][j][e];
      at6(row, r[e]);
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
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float a = cmax_relu ? fmaxf(v[e], 0.f) : v[e];          // (fmaxf(NaN, 0) = 0, as in wino_absmax_kernel)
        mx[e] = max(mx[e], __float_as_uint(a) & 0x7fffffffu);
      }
    }
  }
#pragma unroll
  for (int e = 0; e < 4; ++e)
    if (mx[e]) atomicMax(&sm[n4 * 4 + e], mx[e]);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < N; i += blockDim.x)
    if (sm[i]) atomicMax(&cmax[i], sm[i]);
}

}  // namespace

// launch helper for csrc/winograd.hip (not part of the C ABI): the output transform of one window, merging its channel maxima into cmax
namespace pf_f16x2 {
int launch_output_cmax(const float* M, const pf_conv_params* p, int TH, int TW, long t0, long T, unsigned* cmax, int cmax_relu, hipStream_t st) {
  const long nout = T * (p->Cout / 4);
  hipLaunchKernelGGL(wino_output_cmax_kernel, dim3((unsigned)((nout + 255) / 256)), dim3(256), (size_t)p->Cout * 4, st, M, p->Cout, p->bias,
                     p->act == PF_ACT_RELU ? 1 : 0, static_cast<const float*>(p->res), p->res_ld, static_cast<const float*>(p->res2), p->res2_ld,
                     static_cast<float*>(p->y), p->y_ld, p->B, p->H, p->W, TH, TW, t0, T, cmax, cmax_relu);
  return hipGetLastError() == hipSuccess ? PF_OK : PF_ERR_LAUNCH;
}
}  // namespace pf_f16x2

// the batched product of pf_gemm_f16x2_points on 128 x 128 tiles (same operands, same result bits)
extern "C" int pf_gemm_f16x2_points128(const pf_conv_params* p, const int* col_exp, int grid_cap, void* stream) {
  if (const int rc = f16x2_points_envelope("pf_gemm_f16x2_points128", p, col_exp)) return rc;
  constexpr int smem = 3 * 2 * (128 + 128) * 64;
  static std::atomic<unsigned long long> done{0};
  const long M = (long)p->B * p->OH * p->OW;
  const int mt = (int)((M + 127) / 128), nt = (p->Cout + 127) / 128;
  const long total = (long)mt * nt * (p->batch > 1 ? p->batch : 1);
  const int grid = pf_launch::persist_grid(pf_cu_count(), grid_cap, total, PF_GRID_CAP | PF_GRID_FLOOR8);
  if (grid < 0) return pf_refuse("pf_gemm_f16x2_points128", "argument outside the envelope (include/pf_hip.h)");
  if (!pf_ensure_dynamic_lds(done, smem, gemm_f16x2_persist128_kernel)) return PF_ERR_LAUNCH;
  pf_conv_params q = *p;
  q.scale = reinterpret_cast<const float*>(col_exp);     // (int32 exponents; the kernel's epilogue reads them as such)
  hipLaunchKernelGGL(gemm_f16x2_persist128_kernel, dim3((unsigned)grid), dim3(512), smem, reinterpret_cast<hipStream_t>(stream), q, mt, nt, (int)total);
  return hipGetLastError() == hipSuccess ? PF_OK : PF_ERR_LAUNCH;
}
