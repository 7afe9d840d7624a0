/* C ABI of libpf_hip.so -- the MI355X (gfx950) kernels behind PatchFusion's tiled-inference hot path.
 *
 * Plain pointers and sizes only (no torch types).  Every entry point launches asynchronously on
 * the hipStream_t passed as `stream` (a void*), borrows the device pointers for the duration of
 * the call and returns an int status (PF_OK = 0; message via pf_last_error()).  The Python host
 * (patchfusion_amd/hip_ops.py) binds these with ctypes; INTEGRATION.md shows the stub a reference
 * maintainer would add.  Each group cites the reference interface (file:line under the reference
 * repo) whose stock PyTorch / torchvision / cuDNN op it replaces.
 *
 * dtype: 0 = float32 activations + f32-input MFMA ("exact"), 1 = bf16 activations + bf16 MFMA with
 * f32 accumulation ("fast").  All activation tensors are NHWC with an explicit pixel stride `ld`
 * (elements) so producers write directly into channel slices of concat buffers.
 */
#ifndef PF_HIP_H
#define PF_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PF_DTYPE_F32 0
#define PF_DTYPE_BF16 1

#define PF_ACT_NONE 0
#define PF_ACT_RELU 1
#define PF_ACT_GELU 2      /* exact erf GELU (nn.GELU default) */
#define PF_ACT_SOFTPLUS 3  /* nn.Softplus(beta=1, threshold=20) */

const char* pf_last_error(void);
int pf_version(void);

/* ---- implicit-GEMM convolution / linear layer on the matrix cores --------------------------
 * y[b,oy,ox,n] = epi( sum_{ky,kx,c} x[b, oy*stride-pad+ky, ox*stride-pad+kx, c] * w[n,ky,kx,c] )
 * epi(v) = (act(v + bias[n]) * scale[n]) + res[...] + res2[...]
 * Replaces: F.conv2d / nn.Linear / nn.ConvTranspose2d(k==s) + fused bias/ReLU/GELU/LayerScale/
 * residual everywhere on the path: dinov2/layers/attention.py:51,60, mlp.py:35-41, block.py:82-107,
 * patch_embed.py:76, depth_anything/dpt.py:30-63,87-95, blocks.py:53-59,117,
 * zoedepth layers localbins_layers.py:87-92,112-116, attractor.py:156-161, dist_layers.py:88-95,
 * estimator/models/patchfusion.py:121-127, blocks/guided_fusion_model.py:41-48,59-66,
 * blocks/swin_layers.py:39-41,125-127.
 * Weights are pre-packed by the host as [w_rows][Kpad], zero padded, in `dtype`; K order = (ky,kx,c) (`korder` 0) or, for
 * float32 k x k layers with Cin % 32 == 0, chunk-major (c/32, ky, kx, c%32) (`korder` 1: all taps of one 32-channel chunk
 * are adjacent, so the re-reads of an input pixel hit L2) -- patchfusion_amd/packing.py.
 */
typedef struct {
  const void* x; int x_ld; int B, H, W, Cin; /* Cin: valid input channels, multiple of 8 (zero weights on pad) */
  const void* w; int w_rows; int Kpad;      /* Kpad multiple of 64 (bf16) / 32 (f32) elements */
  const float* bias; const float* scale;    /* [Cout] or NULL (indexed by output channel) */
  const void* res; int res_ld; const void* res2; int res2_ld; /* residual(s), NHWC like y, or NULL */
  void* y; int y_ld; int OH, OW, Cout;      /* Cout: GEMM N = channels stored, multiple of 4 */
  int KH, KW, stride, pad;
  int act;       /* PF_ACT_* */
  int relu_in;   /* apply ReLU to x on load (ResidualConvUnit, blocks.py:78,83) */
  int out_f32;   /* store float32 even when dtype == bf16 (bins-head tensors) */
  int shuffle;   /* 1 = none; s>1: ConvTranspose2d(kernel=stride=s): N = s*s*Cout_t, y is [B,OH*s,OW*s,Cout_t]; 0 and negative values are refused */
  int dtype;
  int korder;    /* K order of w: 0 = (ky,kx,c); 1 = (c/32, ky, kx, c%32), f32 only, Cin % 32 == 0 (see packing.py) */
  int batch;     /* > 1: that many independent GEMM planes in ONE launch (float32, no bias / scale / residual): plane k reads
                    x + k*x_bstride, w + k*w_bstride and writes y + k*y_bstride (strides in elements); 0 / 1 = a single plane.
                    Used for the (m+2)^2 transform points of a Winograd layer (pf_conv_winograd). */
  long x_bstride, w_bstride, y_bstride;
  const int* col_exp;  /* fp16x2 linears only (pf_gemm_f16x2): int32 column exponents f_n [w_rows], y = ldexp(acc, f_n) before the epilogue */
  const int* out_exp;  /* fp16x2 linears with fp16x2 planes out: int32 exponents of the consumer's input channels [Cout] */
} pf_conv_params;
/* pf_conv: Refused (PF_ERR_ARG): a null p / x / w / y; x or w off a 16-byte boundary, y off four of its elements, bias / scale / res / res2 off one
 * element (residual views one element off a vector boundary are computed); a dtype other than 0 / 1, an act outside PF_ACT_*, shuffle < 1 (1 = none),
 * batch < 0 or > 65535; B, H, W, OH, OW, KH, KW, stride not positive, pad < 0, OH / OW other than (H + 2 pad - KH) / stride + 1 and (W + 2 pad - KW) /
 * stride + 1; Cin not a positive multiple of the 16-byte vector, x_ld not such a multiple or below Cin; Cout not a positive multiple of 4, y_ld / res_ld
 * / res2_ld not multiples of 4 or below the channels of a pixel (Cout, Cout / s^2 for y under the pixel shuffle); Kpad not a positive multiple of the
 * 128-byte chunk or below KH KW Cin; w_rows < Cout; more than 16 taps; B OH OW >= 2^31; korder other than 0, or 1 outside float32 with Cin % 32 == 0;
 * batch > 1 with bf16, shuffle, bias, scale, a residual or a missing plane stride; shuffle > 1 with a filter other than 1 x 1, a residual, or Cout / s^2
 * not a multiple of 4. */
int pf_conv(const pf_conv_params* p, void* stream);
/* timing helper for the roofline entry of bench.py: runs `iters` launches bracketed by HIP events on
 * `stream`, returns the average milliseconds per launch in *ms */
/* pf_conv_timed: Refused (PF_ERR_ARG): as pf_conv, and a null ms or iters <= 0. */
int pf_conv_timed(const pf_conv_params* p, int iters, float* ms, void* stream);
/* Introspection for the tests: the kernel variant that the calling thread's last pf_conv launched (0 before the first launch).  Read-only; no
 * dispatch rule reads it and nothing is launched.  code = family * 10^8 + shape * 100 + shuffle * 10 + relu_in, shuffle = 0 | 2 | 4 ..., with
 *   family 1: conv3x3_halo_kernel<WN, FM, FN>        shape = WN * 100 + FM * 10 + FN      (121, 122, 242, 243)
 *   family 2: gemm_persist_kernel<BM, BN>             shape = BM * 1000 + BN               (128128, 128096, 128064, 144128, 144064, 256128)
 *   family 3: conv_igemm_big_kernel (256 x 128)       shape = 256128
 *   family 4: conv_igemm_kernel<bf16, BM, BN>         shape = BM * 1000 + BN               (128128, 128096, 128064, 256032, 256016)
 *   family 5: conv_igemm_kernel<float, BM, BN>        shape = BM * 1000 + BN               (the above, 64064, 256256); a layer split into a body
 *             and a remainder launch reports the remainder's tile */
int pf_conv_last_variant(void);

/* Winograd F(m x m, 3 x 3), m = 2 or 4, for float32 3x3 / stride 1 / pad 1 layers (same reference layers as pf_conv): `p` describes
 * the convolution exactly as for pf_conv (x, bias, res, res2, y, act NONE | RELU, relu_in; p->w is not read; scale must be NULL,
 * Cin % 32 == 0, Cout % 8 == 0); U = the (m+2)^2 transformed filters G g G^T, each packed like a 1x1 pf_conv weight [u_rows][u_kpad]
 * (patchfusion_amd/packing.py winograd_filters); V, M = device workspaces of (m+2)^2 * T * Cin and (m+2)^2 * T * Cout floats,
 * T = B * ceil(H/m) * ceil(W/m).  Input transform -> (m+2)^2 GEMMs through pf_conv -> output transform + epilogue (winograd.hip).
 * m = 2 multiplies 2.25x less than the direct convolution at ~2.5x its float32 rounding error, m = 4 4x less at ~15x. */
/* pf_conv_winograd: Refused (PF_ERR_ARG): a null p / x / y / U / V / M or one of them (or bias / res / res2) off a 16-byte boundary; anything but a
 * float32 3 x 3 / stride 1 / pad 1 layer with shuffle 1 and no scale; B, H, W not positive, OH != H, OW != W; Cin not a positive multiple of 32, Cout of
 * 8; x_ld / y_ld / res_ld / res2_ld not multiples of 4 or below their channels; act other than NONE / RELU; B H W >= 2^31; m other than 2 / 4; u_rows <
 * Cout, u_kpad < Cin or not a multiple of 32. */
int pf_conv_winograd(const pf_conv_params* p, int m, const void* U, int u_rows, int u_kpad, void* V, void* M, void* stream);
/* The same three steps with the transform-domain GEMM in split precision (m = 4): V3 = workspace of 3 x 36 x T x Cin bf16 (the input transform
 * writes the three planes, chunk-major: [3][36][Cin/32][T][32]), U3 = the three bf16 planes of G g G^T, chunk-major [3][36][Cin/32][u_rows][32]
 * (patchfusion_amd/packing.py PackedConv.wino_u3; u_kpad must equal Cin), M = 36 x T x Cout float32; one batched pf_gemm_split3 launch
 * (korder = 6) between the transforms. */
/* pf_conv_winograd_split3: Refused (PF_ERR_ARG): as pf_conv_winograd for p and the pointers; u_rows < Cout, u_kpad != Cin. */
int pf_conv_winograd_split3(const pf_conv_params* p, const void* U3, int u_rows, int u_kpad, void* V3, void* M, void* stream);
/* the same layer `window` Winograd tiles at a time (window % 8 == 0; 0 = all tiles at once): V3 / M then are arenas for ONE window (3 x 36 x window x Cin
 * bf16, 36 x window x Cout float32) that every window reuses -- small windows keep the pair inside the 256 MB memory-side cache.  Tiles are independent:
 * identical results for every window.  With more than one window the output of window k is written before the input of window k + 1 (and its one-pixel
 * halo) is read: x and y must NOT overlap then (PF_ERR_ARG); a residual may alias y (it is read at the pixels being written). */
/* pf_conv_winograd_split3_windowed: Refused (PF_ERR_ARG): as pf_conv_winograd_split3; window < 0 or not a multiple of 8; x and y overlapping when the
 * layer takes more than one window. */
int pf_conv_winograd_split3_windowed(const pf_conv_params* p, const void* U3, int u_rows, int u_kpad, void* V3, void* M, long window, void* stream);
/* fp16x2 form of the same windowed layer (csrc/wino_f16x2.hip): every operand of the transform-domain GEMM is two fp16 planes with a power-of-two
 * scale, three f16 MFMAs per product instead of six bf16 ones.  U = PackedConv.wino_u, float32 [36][u_rows][Cin] (u_kpad == Cin, u_rows % 16 == 0);
 * V2 = arena of 2 x 36 x window x Cin fp16 (window % 8 == 0, 0 = all tiles), M = 36 x window x Cout float32, scratch = pf_wino_f16x2_scratch_bytes
 * bytes (per-call channel maxima of x, the scaled filter planes and their column exponents).  Same argument rules as the bf16x3 entry, the x / y alias
 * refusal included.  pf_conv_winograd_f16x2_supported returns 1 when a call qualifies and the product of the whole layer has an fp16x2 kernel
 * (pf_gemm_f16x2_points_route >= 0: the persistent 192 x 192 or 128 x 128 walk), else 0 -- the caller then takes pf_conv_winograd_split3_windowed. */
/* pf_wino_f16x2_scratch_bytes: Answers 0 for cin <= 0 or u_rows <= 0. */
long pf_wino_f16x2_scratch_bytes(int cin, int u_rows);
/* pf_conv_winograd_f16x2_supported: Answers 0 for every call pf_conv_winograd_f16x2_windowed refuses on account of p, u_rows, u_kpad or window. */
int pf_conv_winograd_f16x2_supported(const pf_conv_params* p, int u_rows, int u_kpad, long window);
/* pf_conv_winograd_f16x2_windowed: Refused (PF_ERR_ARG): as pf_conv_winograd_split3_windowed; u_rows not a multiple of 16; Cin > 8192; a null or
 * misaligned scratch. */
int pf_conv_winograd_f16x2_windowed(const pf_conv_params* p, const void* U, int u_rows, int u_kpad, void* V2, void* M, void* scratch, long window,
                                    void* stream);
/* the same call with the range pass handed from layer to layer: cmax_in = the channel maxima of x (uint32 [Cin] float bits, of relu(x) when
 * p->relu_in) as the producer's output transform merged them, or NULL = run the range pass; cmax_out = NULL or a uint32 [Cout] buffer into which this
 * layer's output transform merges max |y| per channel (of max(y, 0) when cmax_out_relu != 0); it is zeroed once per call, every window accumulates
 * into it, and it equals what the range pass computes on y bit for bit.  y is bit-identical with and without cmax_out. */
/* pf_conv_winograd_f16x2_windowed_ex: Refused (PF_ERR_ARG): as pf_conv_winograd_f16x2_windowed; cmax_in / cmax_out off a 4-byte boundary; cmax_out ==
 * cmax_in. */
int pf_conv_winograd_f16x2_windowed_ex(const pf_conv_params* p, const void* U, int u_rows, int u_kpad, void* V2, void* M, void* scratch, long window,
                                       const void* cmax_in, void* cmax_out, int cmax_out_relu, void* stream);
/* pf_conv_winograd_split3_windowed as such a producer */
/* pf_conv_winograd_split3_windowed_ex: Refused (PF_ERR_ARG): as pf_conv_winograd_split3_windowed; cmax_out off a 4-byte boundary. */
int pf_conv_winograd_split3_windowed_ex(const pf_conv_params* p, const void* U3, int u_rows, int u_kpad, void* V3, void* M, long window, void* cmax_out,
                                        int cmax_out_relu, void* stream);
/* the range pass alone (the reference of the hand-over): cmax uint32 [C] must be zeroed by the caller; x float32 [P][x_ld], C % 4 == 0 */
/* pf_wino_absmax: Refused (PF_ERR_ARG): null pointers, x off a 16-byte or cmax off a 4-byte boundary; P <= 0; C not a positive multiple of 4; x_ld not a
 * multiple of 4 or below C. */
int pf_wino_absmax(const void* x, int x_ld, long P, int C, int relu_in, void* cmax, void* stream);
/* its batched product alone: x / w = two fp16 planes each, chunk-major (korder = 6, batch = transform points, no epilogue), y float32 =
 * ldexp(sum, col_exp[z][n]) with col_exp int32 [batch][w_rows] */
/* pf_gemm_f16x2_points: Refused (PF_ERR_ARG): as pf_gemm_split3 for the linear-layer rules; a null or 16-byte-misaligned x / w / y / col_exp; korder !=
 * 6, out_f32 == 0; x_ld != Cin, Kpad != Cin, w_rows % 4; any epilogue (bias, scale, res, res2, act); M * 64 or w_rows * 64 >= 2^31; fewer than 8 tiles
 * in the launch. */
int pf_gemm_f16x2_points(const pf_conv_params* p, const int* col_exp, int grid_cap, void* stream);
/* the same product on 128 x 128 tiles (csrc/wino_f16x2_n256.hip; the 256-column layers): same operands, same result bits */
/* pf_gemm_f16x2_points128: Refused (PF_ERR_ARG): as pf_gemm_f16x2_points (fewer than 8 tiles are accepted). */
int pf_gemm_f16x2_points128(const pf_conv_params* p, const int* col_exp, int grid_cap, void* stream);
/* the same product on 160 x 256 tiles (csrc/wino_f16x2_t160.hip: the points mode of the tile of the ViT linears): same operands, same result bits;
 * grid: PF_GRID_CAP | PF_GRID_FLOOR8 */
/* pf_gemm_f16x2_points160: Refused (PF_ERR_ARG): as pf_gemm_f16x2_points (fewer than 8 tiles are accepted). */
int pf_gemm_f16x2_points160(const pf_conv_params* p, const int* col_exp, int grid_cap, void* stream);
/* whether the fp16x2 product of a three-step Winograd layer runs on that tile (1) or on the form pf_gemm_f16x2_points_route names (0); p = the
 * product of the WHOLE layer (M = all its Winograd tiles), so the answer does not depend on the window; no launch.  At default switches: 1 for
 * Cout == 256 with Cin >= 512, else 0 (profiles/r14_wino_t160_ab.md, r14_wino_t160_image_ab.md).  PF_WINO_F16_TILE (read per
 * call): 0 = never, 1 = everywhere, 2 = the 768-column class alone (Cout == 768, Cin >= 512), 3 = the 256-column class alone (Cout == 256,
 * Cin >= 512); 2 and 3 exist for the image-pass A/B of one class at a time.  The route queries above keep their values: this decision is separate
 * from them. */
/* pf_wino_f16x2_tile_route: Answers -1 for a null p or cus <= 0. */
int pf_wino_f16x2_tile_route(const pf_conv_params* p, int cus);
/* which of the two runs the product of a whole layer on a chip of `cus` compute units: PF_S3_ROUTE_PERSIST192, PF_S3_ROUTE_PERSIST128, or -1 when
 * the layer stays on three bf16 planes (pf_gemm_split3_route gives TILE64 / TILE128, or PF_WINO_F16X2_N256=0 for the 128-tile layers, or a 128-tile layer outside the measured rule -- K >= 512 and >= 4096 tiles; =3: every one); no launch */
/* pf_gemm_f16x2_points_route: Answers -1 for a null p or cus <= 0. */
int pf_gemm_f16x2_points_route(const pf_conv_params* p, int cus);
/* the same rule for a layer whose channel maxima are handed in (maxima_given != 0: no memset, no range pass).  At default switches the answer does not
 * depend on maxima_given (the wider rule measured no gain in the image pass, profiles/r12_cmax_image_ab.md); under PF_WINO_F16X2_N256=5 the 128-tile
 * layers with given maxima take fp16x2 from K >= 256 and 2128 Winograd tiles on (profiles/r11_n256_sweep.md, column "maxima given") */
/* pf_gemm_f16x2_points_route_ex: Answers -1 for a null p or cus <= 0. */
int pf_gemm_f16x2_points_route_ex(const pf_conv_params* p, int cus, int maxima_given);
/* pf_conv_winograd_f16x2_supported by that rule, for a call that will pass cmax_in (maxima_given != 0) */
/* pf_conv_winograd_f16x2_supported_ex: Answers 0 as pf_conv_winograd_f16x2_supported. */
int pf_conv_winograd_f16x2_supported_ex(const pf_conv_params* p, int u_rows, int u_kpad, long window, int maxima_given);
/* fp16x2 linear layer (the ViT block linears; packing.pack_conv_f16x2): x = two fp16 planes, chunk-major [2][K/32][M][32], holding x / 2^e_k;
 * w = two fp16 planes [2][K/32][w_rows][32] holding W[n][k] 2^(e_k - f_n); korder must be 6 (| 16, see below).  p->col_exp = f_n [w_rows] (required).
 * The persistent 192 x 192 kernel sums the three products hh, hl, lh in float32, applies ldexp(acc, f_n) and then the pf_conv epilogue
 * (bias -> act -> scale -> res -> res2, all float32), and stores one of: float32 [M][y_ld] (out_f32); three bf16 planes, row-major [3][M][y_ld]
 * (y_bstride); or, with korder bit 16, two fp16 chunk-major planes [2][Cout/32][M][32] of y / 2^out_exp[n] (y_ld == Cout, Cout % 32 == 0,
 * p->out_exp required); or, with korder bit 32, two fp16 ROW-major planes [2][M][y_ld] (y_bstride) of y / 2^out_exp[n] (p->out_exp required):
 * q / k / v for pf_vit_attention_f16x2, which reads token rows.  Bits 16 and 32 exclude each other.  No batch.
 * float32 output also has a 160 x 256 tile form (csrc/gemm_f16x2_t160.hip: same products in the same order, same bits); pf_gemm_f16x2_route
 * tells which one a call runs. */
/* pf_gemm_f16x2: Refused (PF_ERR_ARG): as pf_gemm_split3 for the linear-layer rules and the alignment of x / w / y / bias / scale / res / res2; a null
 * or misaligned col_exp (out_exp with the plane outputs); batch > 1; korder other than 6 (| 16 | 32), bits 16 and 32 together, or either with float32
 * output; x_ld != Cin, Kpad != Cin, w_rows % 4; korder bit 16 with y_ld != Cout or Cout % 32; M * 64 or w_rows * 64 >= 2^31. */
int pf_gemm_f16x2(const pf_conv_params* p, void* stream);
/* which tile form pf_gemm_f16x2 runs on a chip of `cus` compute units (no launch, no GPU needed): PF_S3_ROUTE_PERSIST192 or PF_S3_ROUTE_TILE160.
 * The 160 x 256 form takes float32-output calls whose rounds of tiles x tile cost (60 MFMAs per chunk and wave against 54) come out lower:
 * ceil(t160 / cus) * 60 < ceil(t192 / cus) * 54.  PF_F16_TILE (read per call): 0 = 192 x 192 everywhere, 1 = 160 x 256 wherever it is legal
 * (float32 output).  -1 for a NULL p or cus <= 0. */
/* pf_gemm_f16x2_route: Answers -1 for a null p or cus <= 0. */
int pf_gemm_f16x2_route(const pf_conv_params* p, int cus);

/* FUSED Winograd F(4x4, 3x3) (csrc/wino_fused.hip): the same layers in ONE kernel -- the transformed input and the transform-domain
 * products never exist in HBM.  `p` as for pf_conv_winograd (p->w is not read); `up` = the filters in MFMA fragment order
 * [nnb][Cin/8][36][2][64][4] floats (patchfusion_amd/packing.py winograd_filters_fused), nnb = ceil(Cout/64); `gs` & 0xffff =
 * super-tiles (32 output tiles: 4 x 8 or 8 x 4, picked for the least padding) per block group (L2 locality knob, >= 1), `gs` >> 16 = 0
 * or a forced super-tile width 8 | 4 (tuning aid).  Needs Cin % 16 == 0, Cin >= 32, Cout % 4 == 0, B*H*W*x_ld < 2^31:
 * pf_conv_winograd_fused_supported(p) returns 1 when `p` qualifies, else 0 (callers then take pf_conv_winograd / pf_conv). */
/* pf_conv_winograd_fused_supported: Answers 0 also for B, H, W not positive, shuffle != 1, x_ld < Cin, y_ld / res_ld / res2_ld < Cout and x / y / bias /
 * res / res2 off a 16-byte boundary. */
int pf_conv_winograd_fused_supported(const pf_conv_params* p);
/* pf_conv_winograd_fused: Refused (PF_ERR_ARG): a null p / x / y / up; whatever pf_conv_winograd_fused_supported answers 0 to (which now includes B, H,
 * W not positive, x_ld < Cin, y_ld / res_ld / res2_ld < Cout, shuffle != 1 and x / y / bias / res / res2 off a 16-byte boundary); up off a 16-byte
 * boundary; nnb != ceil(Cout / 64); gs < 0 or a forced super-tile width other than 0 / 4 / 8. */
int pf_conv_winograd_fused(const pf_conv_params* p, const void* up, int nnb, int gs, void* stream);
/* timing helper like pf_conv_timed: `iters` launches bracketed by HIP events on `stream` */
/* pf_conv_winograd_fused_timed: Refused (PF_ERR_ARG): as pf_conv_winograd_fused, and a null ms or iters <= 0. */
int pf_conv_winograd_fused_timed(const pf_conv_params* p, const void* up, int nnb, int gs, int iters, float* ms, void* stream);

/* ---- split-precision linear layer (csrc/gemm_split3.hip; the float32 mode's ViT block linears) --------------------------------------------
 * float32-grade y = epi(x . w^T) on the bf16 matrix cores: x and w are given as THREE bf16 planes each (x = x_h + x_m + x_l, round-to-
 * nearest splits) and the six leading partial products are accumulated in float32.  `p` as for pf_conv with KH = KW = 1: x = planes
 * [3][M][x_ld] bf16 (plane stride x_bstride elements), w = planes [3][w_rows][Kpad] bf16 (w_bstride; packing.pack_conv_split3), Cin % 32
 * == 0, bias / scale / res / res2 float32; y = float32 [M][y_ld] when out_f32 != 0, else three bf16 planes [3][M][y_ld] (y_bstride) for a
 * following split GEMM.  Same reference layers as pf_conv's linear use (attention.py:51,60, mlp.py:35-41).
 * p->korder here selects the OPERAND layout: bit 1 (value 2) = every x plane is chunk-major [Cin/32][M][32] (x_ld must equal Cin), bit 2
 * (value 4) = every w plane is chunk-major [Cin/32][w_rows][32] (Kpad must equal Cin): each 32-deep K chunk of all rows is one contiguous
 * slab, which is what the kernel's 1-KiB LDS-DMA pieces want (whole cache lines); bit 3 (value 8) = the three-plane OUTPUT (out_f32 == 0) is
 * written chunk-major [Cout/32][M][32] (y_ld must equal Cout, Cout % 32 == 0) for a following split GEMM.  p->batch > 1: that many independent planes in one launch
 * (block k of every x / w plane, float32 output block k, no epilogue) -- the transform points of pf_conv_winograd_split3.
 * Kernel choice is internal and result-identical (same chunk order, same six terms per accumulator): 64 x 128 tiles below one round of tiles,
 * one 128 x 128 tile per block, or -- from two rounds of tiles on -- a PERSISTENT kernel (one block per CU walks its tiles) with 128 x 128 tiles
 * on a three-slot LDS ring or 192 x 192 tiles on a two-slot ring, whichever costs fewer rounds x tile cost. */
/* pf_gemm_split3: Refused (PF_ERR_ARG): a null p / x / w / y; x, w, bias, scale, res, res2 off a 16-byte boundary, y off 16 bytes (float32 or chunk-
 * major planes) / 8 bytes (row-major planes); anything but a 1 x 1 / stride 1 / pad 0 / shuffle 1 layer; B, H, W, OH, OW not positive or OH != H, OW !=
 * W; an act outside PF_ACT_*; batch < 0 or > 65535, or > 1 with plane output or an epilogue; Cin not a positive multiple of 32, Kpad not such a multiple
 * or below Cin, x_ld not a multiple of 8 or below Cin; Cout not a positive multiple of 4, y_ld / res_ld / res2_ld not multiples of 4 or below Cout,
 * w_rows < Cout; M >= 2^31; x_bstride / w_bstride not positive multiples of 8, y_bstride (plane output) not a positive multiple of 4 (8 chunk-major);
 * korder bits outside 2 | 4 | 8, bit 2 with x_ld != Cin, bit 4 with Kpad != Cin, bit 8 with float32 output, y_ld != Cout or Cout % 32. */
int pf_gemm_split3(const pf_conv_params* p, void* stream);
/* The same split-precision product for a 1x1 convolution / linear layer whose ACTIVATIONS are plain float32 (round 6; replaces pf_conv's f32-MFMA
 * route for the 1x1 layers of the DPT / metric-bins heads -- external/zoedepth/models/layers/localbins_layers.py:99-117, attractor.py:156-161,
 * base_models/dpt_dinov2/blocks.py (out_conv / projections) -- and the G2L Swin linears, estimator/models/blocks/swin_layers.py:120-128,133-164):
 * `p` exactly as for pf_conv with KH = KW = 1, stride 1, pad 0, shuffle 1, dtype PF_DTYPE_F32 (x float32 [M][x_ld], x_ld % 4 == 0, Cin % 32 == 0;
 * bias / scale / res / res2 / y float32; act, relu_in as pf_conv; p->w is not read); w3 = the weight's three bf16 planes, CHUNK-MAJOR
 * [3][Cin/32][w3_rows][32] (packing.pack_conv_split3(kmajor=True); w3_rows % 16 == 0, >= Cout).  The kernel splits x in its loader (three LDS
 * planes per K chunk), so no producer has to change; error against float64 = pf_gemm_split3's (tests/op_checks.py conv1x1_split3). */
/* pf_conv1x1_split3: Refused (PF_ERR_ARG): a null p / x / y / w3; x, y, w3, bias, scale, res, res2 off a 16-byte boundary; a dtype other than float32;
 * the linear-layer rules of pf_gemm_split3 (1 x 1, sizes positive and consistent, act, shuffle 1); batch > 1; Cin not a positive multiple of 32, x_ld
 * not a multiple of 4 or below Cin; Cout not a positive multiple of 4, y_ld / res_ld / res2_ld not multiples of 4 or below Cout; w3_rows < Cout or not a
 * multiple of 16; M >= 2^31, w3_rows * 64 >= 2^31. */
int pf_conv1x1_split3(const pf_conv_params* p, const void* w3, int w3_rows, void* stream);
/* the same call with the persistent kernels capped at `grid_cap` blocks (0 = one per CU): the CUs left over run the kernels of OTHER streams
 * (the HBM-bound Winograd transforms of the other tile batch) beside the matrix-bound GEMM */
/* pf_gemm_split3_ex: Refused (PF_ERR_ARG): as pf_gemm_split3. */
int pf_gemm_split3_ex(const pf_conv_params* p, int grid_cap, void* stream);
/* which of those kernels a call would run on a chip of `cus` compute units (no launch, no GPU needed: the dispatch rule for host-side tests) */
#define PF_S3_ROUTE_TILE64 0
#define PF_S3_ROUTE_TILE128 1
#define PF_S3_ROUTE_PERSIST128 2
#define PF_S3_ROUTE_PERSIST192 3
#define PF_S3_ROUTE_TILE160 4 /* pf_gemm_f16x2_route only: the persistent 160 x 256 fp16x2 form */
/* pf_gemm_split3_route: Answers -1 for a null p or cus <= 0. */
int pf_gemm_split3_route(const pf_conv_params* p, int cus);
/* how many blocks a persistent GEMM launches for `total` tiles on a chip of `cus` compute units (no launch, no GPU needed: the grid rule for
 * host-side tests).  One block per CU, at most `total`, rounded down to a multiple of 8.  `policy` = the knobs the launcher honours, PF_GRID_CAP
 * (grid_cap > 0 caps the CUs) | PF_GRID_ENV (PF_S3_GRID, read per call, replaces CUs and cap), plus exactly one rule for fewer than 8 blocks:
 *   launcher                                  policy
 *   pf_gemm_split3, 128 and 192 tiles         PF_GRID_CAP | PF_GRID_ENV | PF_GRID_FALLBACK
 *   pf_gemm_f16x2_points                      PF_GRID_CAP | PF_GRID_REFUSE
 *   pf_gemm_f16x2, 192 x 192 tiles            PF_GRID_FLOOR8
 *   pf_gemm_f16x2, 160 x 256 tiles            PF_GRID_ENV | PF_GRID_FLOOR8
 *   pf_gemm_f16x2_points128                   PF_GRID_CAP | PF_GRID_FLOOR8
 *   pf_gemm_f16x2_points160                   PF_GRID_CAP | PF_GRID_FLOOR8
 * Answers the grid; 0 where the launcher falls back to its one-tile kernel; -1 where it refuses (also total > 2^31 - 1). */
#define PF_GRID_CAP 1
#define PF_GRID_ENV 2
#define PF_GRID_FLOOR8 4   /* fewer than 8 blocks: 8 anyway */
#define PF_GRID_FALLBACK 8 /* fewer than 8 blocks: the one-tile kernel runs the call */
#define PF_GRID_REFUSE 16  /* fewer than 8 blocks: PF_ERR_ARG */
/* pf_persist_grid: Answers -1 for cus <= 0, total <= 0, policy bits outside PF_GRID_* or not exactly one of FLOOR8 / FALLBACK / REFUSE. */
int pf_persist_grid(int cus, int grid_cap, long total, int policy);
/* pf_gemm_split3_timed: Refused (PF_ERR_ARG): as pf_gemm_split3, and a null ms or iters <= 0. */
int pf_gemm_split3_timed(const pf_conv_params* p, int iters, float* ms, void* stream);
/* A plain bf16 linear layer (x [M][x_ld] bf16, w from packing.pack_conv, bf16 residuals / output, float32 output when out_f32) through the same
 * ping-pong LDS-DMA pipeline: 256 x 128 tiles, Cin % 64 == 0.  The bf16 mode's ViT block linears at large token counts (same reference layers). */
/* pf_gemm_bf16_pp: Refused (PF_ERR_ARG): a null p / x / w / y; x, w, bias, scale off a 16-byte boundary, y off 16 (float32) / 8 bytes, res / res2 off 8
 * bytes; the linear-layer rules of pf_gemm_split3; a dtype other than bf16; batch > 1; Cin not a positive multiple of 64, x_ld not a multiple of 8 or
 * below Cin, Kpad not a multiple of 8 or below Cin; Cout not a positive multiple of 4, y_ld / res_ld / res2_ld not multiples of 4 or below Cout, w_rows
 * < Cout; M >= 2^31. */
int pf_gemm_bf16_pp(const pf_conv_params* p, void* stream);
/* the split producers of the ViT block: LayerNorm (layers/block.py:88-93 norm1 / norm2) and the attention output (attention.py:58-60)
 * written as three bf16 planes; arguments as pf_layernorm (plain row range) / pf_vit_attention_qkv with the plane stride in elements.
 * kmajor != 0: every output plane is CHUNK-MAJOR [cols/32][rows][32] (rows = all rows of the call), the layout pf_gemm_split3 reads with
 * korder bit 1; kmajor == 0: row-major [rows][ld]. */
/* pf_layernorm_split3: Refused (PF_ERR_ARG): null pointers; x off a 16-byte, y3 off an 8-byte, g / b off a 4-byte boundary; D not a multiple of 8 in [8,
 * 2048]; x_ld / y_ld not multiples of 8 or below D; rows outside [1, 2^31); plane below (rows - 1) y_ld + D or not a multiple of 4; kmajor with D % 32
 * or y_ld != D. */
int pf_layernorm_split3(const float* x, int x_ld, void* y3, int y_ld, long plane, int kmajor, const float* g, const float* b, float eps,
                        long rows, int D, void* stream);
/* LayerNorm as the fp16x2 input of pf_gemm_f16x2: y2 = two fp16 planes, chunk-major [2][D/32][rows][32] (plane = rows * D elements), holding
 * LN(x)[k] / 2^in_exp[k] as h + l (in_exp: int32 [D], packing.pack_conv_f16x2 of the consuming linear) */
/* pf_layernorm_f16x2: Refused (PF_ERR_ARG): null pointers; x / y2 off a 16-byte, in_exp / g / b off a 4-byte boundary; D not a multiple of 32 in [32,
 * 2048]; x_ld not a multiple of 8 or below D; rows outside [1, 2^31). */
int pf_layernorm_f16x2(const float* x, int x_ld, void* y2, const int* in_exp, const float* g, const float* b, float eps, long rows, int D,
                       void* stream);
/* pf_vit_attention_qkv_split3: Refused (PF_ERR_ARG): null pointers; qkv off a 16-byte, out3 off an 8-byte boundary; B, S, Hh not positive; B * Hh >
 * 65535 (grid dimension y); plane below B S Hh 64 or not a multiple of 4. */
int pf_vit_attention_qkv_split3(const void* qkv, void* out3, long plane, int kmajor, int B, int S, int Hh, void* stream);
/* The same attention entirely in split precision: qkv3 = the QKV GEMM's output as three bf16 planes [3][B*S][3*Hh*64] (plane stride plane_in
 * elements), out3 = three bf16 planes [3][B*S][Hh*64] (plane_out); S^T = K.Q^T and O^T = V^T.P^T as six bf16 partial products each with float32
 * accumulation, float32 softmax with the probabilities split in registers (csrc/vit.hip vit_attention_split3_kernel; attention.py:53-60). */
/* pf_vit_attention_split3: Refused (PF_ERR_ARG): null pointers; qkv3 off a 16-byte, out3 off an 8-byte boundary; B, S, Hh not positive; B * Hh > 65535;
 * plane_in below B S Hh 192 or not a multiple of 8, plane_out below B S Hh 64 or not a multiple of 4; 2 plane_in + 65 Hh 192 >= 2^32 (32-bit tile
 * offsets). */
int pf_vit_attention_split3(const void* qkv3, long plane_in, void* out3, long plane_out, int kmajor, int B, int S, int Hh, void* stream);
/* Version 2 of the same operator (csrc/attn_split3.hip; same operands): K / V tiles by LDS-DMA, V^T fragments by the transposing LDS read, 32 (or
 * 16) queries per wave.  queries_per_wave: 16, 32, or 0 = 32 when the launch fills the chip with 128-query blocks, else 16.  schedule: 1 = the
 * two-phase kernel (64-key tiles; bit-identical to pf_vit_attention_split3), 2 = the software-pipelined kernel (32-key blocks, QK / softmax / PV of
 * three consecutive blocks overlapped inside every wave; float32-rounding-identical), 0 = default (2).  Requires S * Hh * 384 bytes < 2^31 (32-bit
 * row offsets inside one image).  Replaces dinov2/layers/attention.py:53-60. */
/* pf_vit_attention_split3_v2: Refused (PF_ERR_ARG): null pointers; qkv3 off a 16-byte, out3 off an 8-byte boundary; B, S, Hh not positive; the plane
 * rules of pf_vit_attention_split3; S * Hh * 384 bytes >= 2^31; queries_per_wave other than 0 / 16 / 32; schedule outside 0 .. 2. */
int pf_vit_attention_split3_v2(const void* qkv3, long plane_in, void* out3, long plane_out, int kmajor, int B, int S, int Hh, int queries_per_wave,
                               int schedule, void* stream);
/* The same attention on TWO SCALED fp16 PLANES (three v_mfma_f32_32x32x16_f16 per product term instead of six bf16 ones; the pipelined kernel's
 * schedule): qkv2 = two fp16 planes [2][B*S][3*Hh*64] (plane stride plane_in elements) holding q[c] / 2^eq[c], k[c] / 2^ek[c], v[d] / 2^ev[d] as h + l
 * (pf_gemm_f16x2 with korder bit 32; packing.vit_attn_f16x2_scales), with eq[c] + ek[c] = qk_exp[h] for EVERY channel c of head h; qk_exp = int32
 * [Hh] on the device, folded into the base-2 softmax scale.  out2 = two fp16 planes, chunk-major [2][Hh*2][B*S][32] (plane stride plane_out elements), holding out[d] / 2^ev[d]: the
 * input of the projection as a pf_gemm_f16x2 layer whose in_exp is ev.  With v_exp3 != NULL (int32 [Hh*64] on the device, ev) the output is
 * written as THREE bf16 planes of out itself, chunk-major [3][Hh*2][B*S][32] -- the input of the projection as a pf_gemm_split3 layer (korder bit 1).
 * Float32 softmax and accumulation.  Requires S * Hh * 384 bytes < 2^31. */
/* pf_vit_attention_f16x2: Refused (PF_ERR_ARG): as pf_vit_attention_split3_v2 for qkv2 / out, B, S, Hh and the planes; a null qk_exp or one off a 4-byte
 * boundary; v_exp3 off a 16-byte boundary. */
int pf_vit_attention_f16x2(const void* qkv2, long plane_in, const int* qk_exp, void* out, long plane_out, const int* v_exp3, int B, int S, int Hh,
                           void* stream);
/* BEiT attention with a per-head relative-position bias (the MiDaS DPT_BEiT_L_384 core that midas.py:189-316 wraps, loaded at midas.py:340;
 * MiDaS v3.1 backbones/beit.py attention_forward + _get_rel_pos_bias): softmax(q k^T / 8 + bias[h, idx(i, j)]) v, operands as
 * pf_vit_attention_split3_v2 (the two-phase kernel, same MFMA arithmetic).  S = th * tw + 1 (cls first); tab [Hh][(2 th - 1)(2 tw - 1) + 3]
 * float32, the bias table already interpolated to the (th, tw) window AND multiplied by log2(e); idx: patch x patch (yi - yj + th - 1)(2 tw - 1)
 * + (xi - xj + tw - 1), cls row -> entry n - 3, cls column -> n - 2, cls x cls -> n - 1.  queries_per_wave 16, 32 or 0 (as v2).  S < 2^20. */
/* pf_vit_attention_split3_rpb: Refused (PF_ERR_ARG): as pf_vit_attention_split3_v2 for the operands, planes and queries_per_wave; a null tab or one off
 * a 4-byte boundary; th, tw not positive, S != th tw + 1, S >= 2^20; a table slice that does not fit 160 KiB of LDS. */
int pf_vit_attention_split3_rpb(const void* qkv3, long plane_in, void* out3, long plane_out, int kmajor, int B, int S, int Hh, const float* tab,
                                int th, int tw, int queries_per_wave, void* stream);
/* The same BEiT attention in the bf16 mode (csrc/vit.hip, the bias form of the 32-queries-per-wave bf16 kernel behind pf_vit_attention; same
 * reference lines as pf_vit_attention_split3_rpb): q, k, vt bf16 exactly as pf_qkv_split writes them with scale = head_dim^-1/2 (Q*scale
 * [B,Hh,S,64], K [B,Hh,S,64], V^T [B,Hh,64,Sp], Sp % 64 == 0, Sp >= S), out bf16 [B*S][Hh*64]; tab float32 [Hh][(2 th - 1)(2 tw - 1) + 3] as
 * above (interpolated, times log2(e)): the kernel forms q.k * log2(e) + tab[h][idx(i, j)] in float32 (the bias is never rounded to bf16) and runs
 * its online softmax on those base-2 logits.  Refused (PF_ERR_ARG): null pointers, S != th * tw + 1, tw < 4, S >= 2^20, Sp not a multiple of 64 or
 * < S, a table slice that does not fit the LDS.  pf_vit_attention is unchanged. */
/* pf_vit_attention_rpb_bf16: Refused (PF_ERR_ARG): also q / k / vt off a 16-byte, out off an 8-byte, tab off a 4-byte boundary; B, Hh not positive; B *
 * Hh > 65535.  The LDS opt-in is kept per device and raised under a lock. */
int pf_vit_attention_rpb_bf16(const void* q, const void* k, const void* vt, void* out, int B, int S, int Sp, int Hh, const float* tab, int th, int tw,
                              void* stream);
/* LDS bytes one block of that kernel reserves: the 32 KiB of K / V^T stages + the largest table slice a 128-query block stages ((y_hi - y_lo + th)
 * (2 tw - 1) + 3 entries, rounded to 16 bytes); -1 for a shape pf_vit_attention_rpb_bf16 refuses.  No launch, no GPU (host-side tests). */
/* pf_vit_attention_rpb_bf16_lds_bytes: Answers -1 for th <= 0, tw < 4, S != th tw + 1 or S >= 2^20. */
int pf_vit_attention_rpb_bf16_lds_bytes(int S, int th, int tw);
/* float32 [rows][x_ld] -> three bf16 planes [3][rows][y_ld], plane stride `plane` elements (the split producers fuse into their stores) */
/* pf_split3: Refused (PF_ERR_ARG): null pointers; x off a 16-byte, y off an 8-byte boundary; cols not a positive multiple of 4; x_ld / y_ld not
 * multiples of 4 or below cols; rows <= 0; plane below (rows - 1) y_ld + cols or not a multiple of 4. */
int pf_split3(const float* x, int x_ld, void* y, int y_ld, long plane, long rows, int cols, void* stream);

/* ---- ViT encoder pieces ---------------------------------------------------------------------- */
/* (x - mean)/std + 14x14/14 patch gather: NCHW float image -> im2col rows [B*th*tw][ld] (K order
 * ky,kx,c).  Replaces depth_anything.py:184-190 (Normalize) + the unfold implied by patch_embed.py:76 */
/* pf_patch_im2col: Refused (PF_ERR_ARG): null pointers or ones off their element size; a dtype other than 0 / 1; B, H, W not positive; H, W not
 * multiples of 14; ld < 588. */
int pf_patch_im2col(const float* img, int B, int H, int W, void* out, int ld, int dtype, void* stream);
/* (x - mean[c])/std[c] + patch x patch / patch gather: NCHW float image -> float32 im2col rows [B*(H/patch)*(W/patch)][ld] (K order ky,kx,c;
 * columns 3 patch^2 .. ld-1 zero).  Replaces midas.py:160-169 (PrepForMidas Normalize(0.5, 0.5)) + the unfold implied by the BEiT patch_embed.proj
 * 16x16/16 conv of the core loaded at midas.py:340.  pf_patch_im2col (14x14, ImageNet statistics) is unchanged. */
/* pf_patch_im2col_norm: Refused (PF_ERR_ARG): null pointers or ones off their element size (mean3 / std3 are HOST arrays of three floats); B, H, W,
 * patch not positive, patch > 1024; H, W not multiples of patch; ld < 3 patch^2; a std that is 0 or NaN. */
int pf_patch_im2col_norm(const float* img, int B, int H, int W, int patch, const float* mean3, const float* std3, float* out, int ld, void* stream);
/* readout 'project' operand rows (MiDaS utils ProjectReadout, the act_postprocess*.0 of the core loaded at midas.py:340): x [B*S][x_ld] float32
 * token rows (cls first) -> y[b*(S-1) + t] = [x[b*S + 1 + t][0:D] | x[b*S][0:D]] (y_ld >= 2 D).  D, x_ld, y_ld multiples of 4; 16-byte pointers. */
/* pf_readout_concat: Refused (PF_ERR_ARG): null pointers or ones off a 16-byte boundary; B < 1, S < 2; D, x_ld, y_ld not positive multiples of 4; x_ld <
 * D; y_ld < 2 D. */
int pf_readout_concat(const float* x, int x_ld, int B, int S, int D, float* y, int y_ld, void* stream);
/* The bf16 mode's forms of those two (csrc/beit_bf16.hip; same reference lines): pf_patch_im2col_norm_bf16 writes bf16 rows [..][ld] -- the float32
 * kernel's value rounded once to nearest even, padding columns zero; pf_readout_concat_bf16 copies bf16 token rows x [B*S][x_ld] into bf16 rows y
 * [B*(S-1)][y_ld] = [token | cls].  D, x_ld, y_ld multiples of 8 there; 16-byte pointers.  Refusals as the float32 forms (PF_ERR_ARG). */
/* pf_patch_im2col_norm_bf16: Refused (PF_ERR_ARG): as pf_patch_im2col_norm. */
int pf_patch_im2col_norm_bf16(const float* img, int B, int H, int W, int patch, const float* mean3, const float* std3, void* out, int ld, void* stream);
/* pf_readout_concat_bf16: Refused (PF_ERR_ARG): as pf_readout_concat with multiples of 8. */
int pf_readout_concat_bf16(const void* x, int x_ld, int B, int S, int D, void* y, int y_ld, void* stream);
/* tokens[b,0,:] = cls + pos[0]; tokens[b,1+t,:] = emb[b*(S-1)+t,:] + pos[1+t]  (vision_transformer.py:222-223) */
/* pf_assemble_tokens: Refused (PF_ERR_ARG): null pointers or ones off their element size; a dtype other than 0 / 1; B, S not positive (S = 1: the cls
 * token alone, emb is not read); D not a positive multiple of 8. */
int pf_assemble_tokens(const void* emb, void* tokens, const float* cls, const float* pos, int B, int S, int D, int dtype,
                       void* stream);
/* LayerNorm over the last dim: y[r] = (x[r]-mu)/sqrt(var+eps)*g+b.  Rows are remapped so that the
 * final `norm` + cls drop of get_intermediate_layers (vision_transformer.py:309-312) is one pass:
 * out row (b, t) <- in row b*in_rows_per_batch + in_row_offset + t, t < out_rows_per_batch. */
/* pf_layernorm: Refused (PF_ERR_ARG): null pointers; x / y off a 16-byte, g / b off a 4-byte boundary; a dtype other than 0 / 1; D not a multiple of 8
 * in [8, 2048]; x_ld / y_ld not multiples of 8 or below D (output rows would overlap); batches, in_rows_per_batch, out_rows_per_batch not positive;
 * in_row_offset < 0 or in_row_offset + out_rows_per_batch > in_rows_per_batch (a read past the batch); 2^31 rows or more. */
int pf_layernorm(const void* x, int x_ld, void* y, int y_ld, const float* g, const float* b, float eps,
                 int batches, int in_rows_per_batch, int in_row_offset, int out_rows_per_batch, int D,
                 int dtype, void* stream);
/* split the fused qkv rows [B*S][3*D] into per-head Q*scale [B,H,S,64], K [B,H,S,64], V^T [B,H,64,Sp] */
/* pf_qkv_split: Refused (PF_ERR_ARG): null pointers or ones off a 16-byte boundary; a dtype other than 0 / 1; B, S, Hh not positive; Sp not a multiple
 * of 64 or below S; B * Hh > 65535 (grid dimension y). */
int pf_qkv_split(const void* qkv, int B, int S, int Hh, void* q, void* k, void* vt, int Sp, float scale,
                 int dtype, void* stream);
/* softmax(q k^T) v per (batch, head), head_dim 64, flash-style on the matrix cores; out [B*S][D].
 * Replaces dinov2/layers/attention.py:53-59 (the materialised N x N scores). */
/* pf_vit_attention: Refused (PF_ERR_ARG): as pf_qkv_split (out: 8 bytes for bf16). */
int pf_vit_attention(const void* q, const void* k, const void* vt, void* out, int B, int S, int Sp, int Hh,
                     int dtype, void* stream);
/* float32 attention straight from the QKV GEMM's rows [B*S][3][Hh][64] (no pf_qkv_split, no Q / K / V^T buffers): softmax(q k^T / 8) v
 * per head, head_dim 64, out [B*S][Hh*64].  Same reference lines as pf_vit_attention (dinov2/layers/attention.py:49-62); base-2 softmax
 * with the hardware exponential (relative error ~1e-7 per probability).  dtype must be PF_DTYPE_F32. */
/* pf_vit_attention_qkv: Refused (PF_ERR_ARG): null pointers or ones off a 16-byte boundary; a dtype other than float32; B, S, Hh not positive; B * Hh >
 * 65535. */
int pf_vit_attention_qkv(const void* qkv, void* out, int B, int S, int Hh, int dtype, void* stream);

/* ---- G2L (Swin window attention) -------------------------------------------------------------- */
/* LayerNorm(norm1) -> zero pad to a multiple of 12 -> cyclic shift -> window partition
 * (swin_layers.py:223-244): x [B,H,W,C] tokens -> xw [B*nW*144][C] */
/* pf_swin_ln_partition: Refused (PF_ERR_ARG): null pointers; x / xw off a 16-byte, g / b off a 4-byte boundary; a dtype other than 0 / 1; B, H, W not
 * positive; C / 8 not a power of two in [1, 64]; x_ld not a multiple of 8 or below C; shift outside [0, 12); 2^31 padded tokens or more. */
int pf_swin_ln_partition(const void* x, int x_ld, void* xw, const float* g, const float* b, float eps,
                         int B, int H, int W, int C, int shift, int dtype, void* stream);
/* window attention with relative-position bias and shift mask (swin_layers.py:133-164,327-345);
 * qkv [B*nW*144][3C] -> out [B*nW*144][C]; bias_table [529][heads] float */
/* pf_swin_window_attention: Refused (PF_ERR_ARG): null pointers; qkv / out off a 16-byte, bias_table off a 4-byte boundary; a dtype other than 0 / 1; B,
 * Hp, Wp not positive, Hp / Wp not multiples of 12; C not a positive multiple of 8; heads outside [1, 65535] or not dividing C (heads = 0 used to divide
 * by zero on the host); a head_dim C / heads outside {2, 4, 8, 16, 32}; shift outside [0, 12). */
int pf_swin_window_attention(const void* qkv, void* out, const float* bias_table, int B, int Hp, int Wp,
                             int C, int heads, int shift, int dtype, void* stream);
/* window reverse + un-shift + crop + residual (swin_layers.py:250-263): y = shortcut + proj[win(tok)] */
/* pf_swin_unpartition_add: Refused (PF_ERR_ARG): null pointers or ones off a 16-byte boundary; a dtype other than 0 / 1; B, H, W not positive; C not a
 * positive multiple of 8; s_ld / y_ld not multiples of 8 or below C; shift outside [0, 12). */
int pf_swin_unpartition_add(const void* proj, const void* shortcut, int s_ld, void* y, int y_ld, int B, int H,
                            int W, int C, int shift, int dtype, void* stream);
/* x[b,t,:] += pos[t,:]  (absolute_pos_embed, swin_layers.py:419-420); pos float [T][C] */
/* pf_add_rowwise: Refused (PF_ERR_ARG): null pointers; x off a 16-byte, pos off a 4-byte boundary; a dtype other than 0 / 1; B, T not positive; C not a
 * positive multiple of 8; x_ld not a multiple of 8 or below C. */
int pf_add_rowwise(void* x, int x_ld, const float* pos, int B, int T, int C, int dtype, void* stream);

/* ---- memory-bound image ops --------------------------------------------------------------------- */
/* bilinear, align_corners=True (F.interpolate; used at dpt.py:126,154, blocks.py:147,
 * attractor.py:179,186, zoedepth_v1.py:204-214, guided_fusion_model.py:97,192).
 * y[b,oy,ox, 0..C) = (add ? add[...] : 0) + interp(x).  NHWC both sides. */
/* pf_resize_bilinear: Refused (PF_ERR_ARG): null x / y; x, y, add off a 16-byte boundary; a dtype other than 0 / 1; B, H, W, OH, OW not positive; C not
 * a positive multiple of 8; x_ld / y_ld (add_ld with add) not multiples of 8 or below C; 2^31 (batch, row) pairs or items of a row. */
int pf_resize_bilinear(const void* x, int x_ld, int B, int H, int W, int C, void* y, int y_ld, int OH, int OW,
                       const void* add, int add_ld, int in_f32, int out_f32, int dtype, void* stream);
/* nsrc (2 or 3) bilinear align_corners=True resizes of NHWC tensors xs[i] [B,Hs[i],Ws[i],Cs[i]] (pixel stride lds[i]) written to
 * consecutive channel ranges of y [B,OH,OW, sum Cs] (pixel stride y_ld): the Upv1 concat of guided_fusion_model.py:96-99
 * (cat[feat_enc_resized, up(temp), up(guide)]) in one launch.  All tensors in `dtype`.  The five arrays are HOST arrays. */
/* pf_resize_concat: Refused (PF_ERR_ARG): null arrays, sources or y; a source or y off a 16-byte boundary; nsrc outside 2 .. 3; a dtype other than 0 /
 * 1; per source the rules of pf_resize_bilinear; y_ld not a multiple of 8 or below the sum of the channels. */
int pf_resize_concat(const void* const* xs, const int* lds, const int* Hs, const int* Ws, const int* Cs, int nsrc, int B,
                     void* y, int y_ld, int OH, int OW, int dtype, void* stream);
/* planar float version for the image crops (depth_anything/transform.py:127-129 applied per tile,
 * baseline_pretrain.py:258-264): img [3][H][W] float -> out [P][3][oh][ow] float; boxes int [P][4]=(x0,y0,x1,y1) */
/* pf_crop_resize_planar: Refused (PF_ERR_ARG): null pointers or ones off a 4-byte boundary; C, H, W, P, oh, ow not positive; 2^29 boxes or more.  (The
 * boxes live on the device: they must lie inside the image.) */
int pf_crop_resize_planar(const float* img, int C, int H, int W, const int* boxes, int P, float* out, int oh, int ow,
                          void* stream);
/* torchvision.ops.roi_align(aligned=True, sampling_ratio=-1) (patchfusion.py:247,251;
 * guided_fusion_model.py:202). feat [Bf,H,W,C] NHWC; rois float [K][5] = (batch, x1,y1,x2,y2);
 * out [K,oh,ow,C] (ld y_ld).  in_f32/out_f32 select float storage for the depth map. */
/* pf_roi_align: Refused (PF_ERR_ARG): null pointers; rois off a 4-byte boundary; a dtype other than 0 / 1; Bf, H, W, C, K, oh, ow not positive;
 * spatial_scale not positive; C = 1 (planar) without in_f32 and out_f32 or with feat / y off a 4-byte boundary; C > 1 not a multiple of 8, f_ld / y_ld
 * not multiples of 8 or below C, feat / y off a 16-byte boundary; K * oh >= 2^31.  The batch index of an RoI lives on the device: the kernels CLAMP it
 * to [0, Bf) (NaN -> 0). */
int pf_roi_align(const void* feat, int f_ld, int Bf, int H, int W, int C, const float* rois, int K, void* y,
                 int y_ld, int oh, int ow, float spatial_scale, int in_f32, int out_f32, int dtype, void* stream);
/* nn.MaxPool2d(2) (guided_fusion_model.py:78) */
/* pf_maxpool2: Refused (PF_ERR_ARG): null pointers or ones off a 16-byte boundary; a dtype other than 0 / 1; B not positive, H or W < 2 (odd sizes
 * floor); C not a positive multiple of 8; x_ld / y_ld not multiples of 8 or below C. */
int pf_maxpool2(const void* x, int x_ld, int B, int H, int W, int C, void* y, int y_ld, int dtype, void* stream);
/* channel-slice copy y[..., 0..C) = x[..., 0..C) with optional dtype change */
/* pf_copy_channels: Refused (PF_ERR_ARG): null pointers or ones off a 16-byte boundary; a dtype other than 0 / 1; npix <= 0; C not a positive multiple
 * of 8; x_ld / y_ld not multiples of 8 or below C. */
int pf_copy_channels(const void* x, int x_ld, void* y, int y_ld, long npix, int C, int in_f32, int out_f32,
                     int dtype, void* stream);
/* The same four calls as PRODUCERS of an fp16x2 Winograd layer's range pass (pf_conv_winograd_f16x2_windowed_ex cmax_in): with cmax != NULL (float32
 * calls only, dtype == PF_DTYPE_F32, else PF_ERR_ARG) the kernel also merges, for every channel it writes, the maximum over the pixels it writes of
 * (float bits & 0x7fffffff) of the value as stored into cmax[channel], uint32, indexed by the channel position in y as given -- the producers of one
 * concat buffer pass cmax + their channel offset and fill one vector.  cmax is NOT zeroed here: the caller zeroes it once before the first producer.
 * Unsigned maxima are order-free, so the vector equals pf_wino_absmax over the finished channels bit for bit; y is bit-identical with and without
 * cmax.  cmax == NULL: exactly the plain call. */
/* n uint32 words at p = 0, one memset on `stream` (the maxima vector before its first producer) */
/* pf_zero_u32: Refused (PF_ERR_ARG): a null p or one off a 4-byte boundary; n <= 0. */
int pf_zero_u32(void* p, long n, void* stream);
/* pf_resize_bilinear_ex: Refused (PF_ERR_ARG): as pf_resize_bilinear; cmax off a 4-byte boundary or given to a call that is not float32. */
int pf_resize_bilinear_ex(const void* x, int x_ld, int B, int H, int W, int C, void* y, int y_ld, int OH, int OW,
                          const void* add, int add_ld, int in_f32, int out_f32, int dtype, void* cmax, void* stream);
/* pf_resize_concat_ex: Refused (PF_ERR_ARG): as pf_resize_concat; cmax off a 4-byte boundary or given to a call that is not float32. */
int pf_resize_concat_ex(const void* const* xs, const int* lds, const int* Hs, const int* Ws, const int* Cs, int nsrc, int B,
                        void* y, int y_ld, int OH, int OW, int dtype, void* cmax, void* stream);
/* pf_roi_align_ex: Refused (PF_ERR_ARG): as pf_roi_align; cmax off a 4-byte boundary or given to a call that is not float32, to the planar C = 1 form or
 * to C > 8192. */
int pf_roi_align_ex(const void* feat, int f_ld, int Bf, int H, int W, int C, const float* rois, int K, void* y,
                    int y_ld, int oh, int ow, float spatial_scale, int in_f32, int out_f32, int dtype, void* cmax, void* stream);
/* pf_copy_channels_ex: Refused (PF_ERR_ARG): as pf_copy_channels; cmax off a 4-byte boundary or given to a call that is not float32 or has C > 8192. */
int pf_copy_channels_ex(const void* x, int x_ld, void* y, int y_ld, long npix, int C, int in_f32, int out_f32,
                        int dtype, void* cmax, void* stream);
/* fusion-net input cat[coarse_depth_roi, fine_depth, rgb crop] (patchfusion.py:269) -> [B,h,w,8] (3 zero pad) */
/* pf_pack_fusion_input: Refused (PF_ERR_ARG): null pointers; the planes off a 4-byte, y off a 16-byte boundary; a dtype other than 0 / 1; B, h, w not
 * positive. */
int pf_pack_fusion_input(const float* cdepth, const float* fdepth, const float* crops, void* y, int B, int h, int w,
                         int dtype, void* stream);
/* NHWC (ld) <-> NCHW float converters for the module boundary */
/* pf_nhwc_to_nchw_f32: Refused (PF_ERR_ARG): null pointers or ones off their element size; a dtype other than 0 / 1; B, H, W, C not positive; x_ld < C. */
int pf_nhwc_to_nchw_f32(const void* x, int x_ld, float* y, int B, int H, int W, int C, int in_f32, int dtype, void* stream);

/* ---- metric-bins head ----------------------------------------------------------------------------- */
/* AttractorLayerUnnormed (attractor.py:164-208) and the bounded AttractorLayer (:60-136) -- bin_centers_type, zoedepth_v1.py:90-104:
 * c = bilinear_up(b_prev); out = c + reduce_a dist(A_a - c), A_a = A[a * a_stride] + a_eps.
 *   attractor_exp 0: inv_attractor dx / (1 + 300 dx^2) (:44-57), 1: exp_attractor exp(-300 dx^2) dx (:29-41) -- alpha = 300, gamma = 2
 *   are the jit functions' DEFAULTS: the layers call dist() without their own alpha / gamma, the config values never arrive;
 *   kind_sum 0: mean over the attractors, 1: sum;
 *   unnormed layer: A = softplus(mlp), a_stride 1, a_eps 0; bounded layer: A = relu(mlp) (2 n_attr channels), a_stride 2, a_eps 1e-3
 *   (:105-106 overwrites the normalised pair with A[:, :, 0]).  All float. */
/* pf_attractor: Refused (PF_ERR_ARG): null pointers; A off a 4-byte, b_prev / out off a 16-byte boundary; n_bins not a positive multiple of 4; n_attr <
 * 1, a_stride < 1, a_ld < (n_attr - 1) a_stride + 1; B, h, w, hp, wp not positive. */
int pf_attractor(const float* A, int a_ld, int n_attr, int a_stride, float a_eps, int attractor_exp, int kind_sum,
                 const float* b_prev, int hp, int wp, float* out, int B, int h, int w, int n_bins, void* stream);
/* Seed bin centres of the bounded variants: x [npix][x_ld] float = relu(mlp) (bounded) or softplus(mlp), out [npix][n_bins].
 *   bounded   (SeedBinRegressor, localbins_layers.py:52-68): Bn = x + 1e-3; widths = (max - min) Bn / sum(Bn); edges = cumsum([min, widths]);
 *             centre_k = (edge_k + edge_k+1) / 2
 *   normalize (zoedepth_v1.py:178-182, 'normed' and 'hybrid2'): centre -> (centre - min) / (max - min) */
/* pf_seed_bin_centers: Refused (PF_ERR_ARG): null pointers or ones off a 4-byte boundary; npix <= 0; n_bins < 1; x_ld < n_bins. */
int pf_seed_bin_centers(const float* x, int x_ld, float* out, long npix, int n_bins, float min_depth, float max_depth, int bounded,
                        int normalize, void* stream);
/* AttractorLayer tail (attractor.py:132-135): out = clip(sort_k((max - min) * b + min), min, max) per pixel; n_bins <= 64 */
/* pf_bounded_bin_centers: Refused (PF_ERR_ARG): null pointers or ones off a 4-byte boundary; npix <= 0; n_bins outside [1, 64]. */
int pf_bounded_bin_centers(const float* b, float* out, long npix, int n_bins, float min_depth, float max_depth, void* stream);
/* ConditionalLogBinomial tail + expectation (dist_layers.py:29-33,51-69,108-121, zoedepth_v1.py:215-219):
 * pt [B,h,w,4] float = softplus(mlp) ; centers [B,hc,wc,n_bins] float ; depth [B,h,w] float */
/* pf_logbinom_depth: Refused (PF_ERR_ARG): null pointers; pt / depth off a 4-byte, centers off a 16-byte boundary; n_bins not a multiple of 4 in [4,
 * 256]; pt_ld < 4; B, h, w, hc, wc not positive. */
int pf_logbinom_depth(const float* pt, int pt_ld, const float* centers, int hc, int wc, float* depth, int B, int h,
                      int w, int n_bins, float min_temp, float max_temp, void* stream);
/* The whole full-resolution tail of a metric-bins head in one launch (float32): cat[last(32), up(b_embedding)(128), rel?] -> Conv1x1(80) +
 * GELU -> Conv1x1(4) + Softplus -> log-binomial expectation over the up-sampled bin centres (zoedepth_v1.py:207-219, dist_layers.py:97-121).
 * clb: the CLB buffer [B,H,W,clb_ld] whose channels [0,32) hold `last` and (nq == 11) [rel_off, rel_off+8) the relative depth; emb: the
 * low-resolution embedding [B,he,we,128]; w0f / b0 / w2 / b2: packing.bins_tail_weights; centers [B,hc,wc,64]; depth [B,H,W].
 * Replaces pf_resize_bilinear (embedding into the CLB buffer) + two pf_conv + pf_logbinom_depth. */
/* pf_bins_tail: Refused (PF_ERR_ARG): null pointers; clb / emb / w0f / centers off a 16-byte, b0 / w2 / b2 / depth off a 4-byte boundary; clb_ld not a
 * multiple of 4 or below 32; nq other than 10 / 11; with nq = 11 a rel_off that is negative, not a multiple of 4 or with rel_off + 8 > clb_ld; B, H, W,
 * he, we, hc, wc not positive. */
int pf_bins_tail(const float* clb, int clb_ld, int rel_off, const float* emb, int he, int we, const float* w0f, const float* b0,
                 const float* w2, const float* b2, const float* centers, int hc, int wc, float* depth, int B, int H, int W, int nq,
                 float min_temp, float max_temp, void* stream);

/* ---- stitching (estimator/models/utils.py:21-36, baseline_pretrain.py:310-329,205-216) ------------ */
/* init pass: pred[y0+i,x0+j] = depth*mask ; count[...] = mask  (P tiles) */
/* pf_stitch_init: Refused (PF_ERR_ARG): null pointers or ones off a 4-byte boundary; MH, MW, P, ph, pw not positive.  (yx lives on the device: tiles are
 * clipped at every edge of the map.) */
int pf_stitch_init(float* pred, float* count, int MH, int MW, const float* depth, const float* mask, const int* yx,
                   int P, int ph, int pw, void* stream);
/* pf_stitch_finish_init: Refused (PF_ERR_ARG): null pointers or ones off a 4-byte boundary; n <= 0. */
int pf_stitch_finish_init(float* avg, const float* pred, const float* count, long n, void* stream);
/* RunningAverageMap.update restricted to the tile's footprint, tiles applied in order.
 * depth tile is [dh][dw]; when (dh,dw) != (ph,pw) it is nearest-resized (F.interpolate default,
 * baseline_pretrain.py:203) on the fly. */
/* pf_stitch_update: Refused (PF_ERR_ARG): null pointers or ones off a 4-byte boundary; MH, MW, dh, dw, ph, pw not positive; a paste window that starts
 * outside the map (y0 or x0 negative, y0 >= MH, x0 >= MW) -- it is clipped at the far edges only. */
int pf_stitch_update(float* avg, float* count, int MH, int MW, const float* depth, int dh, int dw, const float* mask,
                     int y0, int x0, int ph, int pw, void* stream);
/* RunningAverageMap.resize: avg nearest, count bilinear align_corners */
/* pf_resize_nearest_f32: Refused (PF_ERR_ARG): null pointers or ones off a 4-byte boundary; H, W, OH, OW not positive. */
int pf_resize_nearest_f32(const float* x, int H, int W, float* y, int OH, int OW, void* stream);
/* pf_resize_bilinear_f32: Refused (PF_ERR_ARG): as pf_resize_nearest_f32. */
int pf_resize_bilinear_f32(const float* x, int H, int W, float* y, int OH, int OW, void* stream);

/* ==== input / output side of the path: HBM-bound byte/float streaming ==== */

/* estimator/datasets/general_dataset.py:22-47 read_image(): decoded uint8 HWC RGB -> `img / 255.0` (float64) ->
 * F.interpolate(bicubic, align_corners=True) to image_raw_shape -> float32 CHW planes (`to_tensor(...).float()`, :201).
 * Evaluated in double like the reference; H == OH && W == OW is the exact conversion; reverse_channels = the
 * `[:, :, ::-1]` of the 'u4k' raw-file branch (:24-25). dst is [3][OH][OW]. */
int pf_u8_bicubic_to_f32(const uint8_t* src, int H, int W, int reverse_channels, float* dst, int OH, int OW, void* stream);

/* estimator/utils/color.py:121-128: np.percentile(value[mask], q0 / q1) with mask = (value != invalid_val) when
 * use_invalid, or mask = (invalid_mask[i] == 0) when invalid_mask (n bytes, device) is not NULL -- an explicit mask REPLACES
 * the value test, as in the reference.  Exact order statistics by a three-level radix select on order-preserving integer keys, linear
 * interpolation as numpy 1.24 (the reference's pinned version): index and weight in double, difference in float32.
 * out2 = {percentile q0, percentile q1} (device, float32; NaN when no valid sample).  `workspace`: device buffer of
 * pf_percentile_workspace_bytes() bytes, contents irrelevant on entry. */
int pf_percentile_workspace_bytes(void);
int pf_percentiles_f32(const float* x, long n, float invalid_val, int use_invalid, const uint8_t* invalid_mask, double q0, double q1,
                       float* out2, void* workspace, void* stream);

/* estimator/utils/color.py:130-150 + matplotlib Colormap.__call__(bytes=True): x = (v - vmin)/(vmax - vmin) in float32
 * (v*0 when vmin == vmax), index = trunc(x*N) with matplotlib's under / over / bad rules; lut_rgba has N+3 RGBA rows
 * (N colours, under, over, bad), already `(lut*255).astype(uint8)`; vmin_vmax is a device float[2] (e.g. the output of
 * pf_percentiles_f32); invalid pixels (v == invalid_val, or invalid_mask[i] != 0 when the mask is not NULL) get
 * background_rgba (R | G<<8 | B<<16 | A<<24). out: [n][4].  gamma_corrected (color.py:86-91) is a per-byte map, so the host
 * applies it to the 1 KiB table and the background colour instead of to the image. */
int pf_colorize_f32(const float* depth, long n, const float* vmin_vmax, const uint8_t* lut_rgba, int N, float invalid_val,
                    int use_invalid, const uint8_t* invalid_mask, uint32_t background_rgba, uint8_t* out_rgba, void* stream);

/* estimator/tester/tester.py:75: (depth * 256).astype('uint16') (float32 product, truncation; clamped to [0, 65535]) */
int pf_depth_to_u16(const float* depth, long n, float scale, uint16_t* out, void* stream);

/* estimator/utils/metric.py:87-148 compute_metrics (+ compute_errors :10-52, soft_edge_error :66-71) as one masked
 * reduction over the ground-truth grid [H][W]: pred [ph][pw] is resized on the fly (bilinear, align_corners=False)
 * when the grids differ, clamped to [min_depth, max_depth] (inf -> max, nan -> min); mask = min < gt < max inside the
 * evaluation rectangle rows [crop_y0, crop_y1) x cols [crop_x0, crop_x1) (garg / eigen crops; whole image = 0,H,0,W);
 * edges (or NULL) = disp_gt_edges, non-zero = boundary pixel; additional_mask (or NULL) = [H][W] bytes, zero = excluded
 * (metric.py:128-130, prompt-depth evaluation).  Terms in float32 like numpy, sums in double:
 * out13 = n, #(thresh<1.25), #(<1.25^2), #(<1.25^3), S|gt-p|/gt, S(gt-p)^2/gt, S(gt-p)^2, S(ln gt - ln p)^2,
 *         S(ln p - ln gt), S(ln p - ln gt)^2, S|log10 gt - log10 p|, S soft-edge error, #(mask & edges)   (device)
 * A NaN in gt is invalid itself but makes the soft-edge minimum of its eight neighbours NaN, as np.minimum.reduce does. */
int pf_depth_metrics(const float* gt, int H, int W, const float* pred, int ph, int pw, const float* edges,
                     const uint8_t* additional_mask, float min_depth, float max_depth, int crop_y0, int crop_y1, int crop_x0, int crop_x1,
                     double* out13, void* stream);

/* SILogLoss forward value (estimator/models/losses.py:15-62), the loss of PatchFusion.forward(mode='train') (patchfusion.py:395):
 * pred / target float32 [n] of equal size; ws3 = 3 doubles of device scratch; *loss (device float) = 10*sqrt(var(g) + beta*mean(g)^2)
 * over min_depth < target < max_depth, g = log(pred+1e-7) - log(target+1e-7); 0 when <= 1 valid element. */
int pf_silog_loss(const float* pred, const float* target, long n, float min_depth, float max_depth, float beta, double* ws3,
                  float* loss, void* stream);

/* ---- evaluation side (csrc/evalops.hip): the tensors and images of the reference's evaluation loop that io.hip left on the host ---- */

/* estimator/utils/image_ops.py:25-36 get_boundaries(disp, th, dilation) (duplicated at utils/metric.py:74-85; called by
 * u4k_dataset.py:168 and general_dataset.py:75,84,94,121,133): disp is `planes` float32 planes [H][W], edges the same shape,
 * 0.0f / 1.0f -- the `edges` argument of pf_depth_metrics.  A pixel is 1 when |v - neighbour| > th (float32 difference, strictly
 * greater) for any of its up / down / left / right neighbours inside the image; comparisons with NaN are false.  dilation k > 0 then
 * applies cv2.dilate(edges, ones((k, k)), iterations=1): anchor (k/2, k/2), out[y][x] = max over rows y-k/2 .. y-k/2+k-1 and columns
 * x-k/2 .. x-k/2+k-1 (k = 10: -5 .. +4), pixels outside the image do not contribute.  One launch.  0 <= dilation <= 32 and
 * H * W < 2^31, else PF_ERR_ARG.  disp and edges must not overlap. */
int pf_depth_boundaries(const float* disp, int planes, int H, int W, float th, int dilation, float* edges, void* stream);

/* pf_colorize_f32 with a choice of output layout.  PF_COLOR_RGBA: out is [n][4], the very bytes of pf_colorize_f32.  PF_COLOR_BGR: out is
 * [n][3] = (B, G, R) of the same colours, the background colour included, alpha dropped; out must be 4-byte aligned.  BGR is both
 * estimator/utils/color.py:22-23 (`colorize_infer_pfv1`: `value[:, :, :3][..., ::-1]`; pass use_invalid = 0 and no mask, it has no
 * invalid handling) and estimator/tester/tester.py:69-71 (`colorize(...)[:, :, [2, 1, 0]]`, the array cv2.imwrite takes).
 * The ranges of color.py:10-12 (min, 95th percentile) and :63-64 (min, max) come from pf_percentiles_f32 with use_invalid = 0 and
 * q = 0 / 95 resp. 0 / 100: percentile 0 and 100 of the radix select are the extrema themselves.  Other layouts: PF_ERR_ARG. */
#define PF_COLOR_RGBA 0
#define PF_COLOR_BGR 1
int pf_colorize_f32_ex(const float* depth, long n, const float* vmin_vmax, const uint8_t* lut_rgba, int N, float invalid_val,
                       int use_invalid, const uint8_t* invalid_mask, uint32_t background_rgba, int layout, uint8_t* out, void* stream);

/* ---- PNG encoding of the saved images (csrc/png.hip, csrc/png_huff.h): estimator/tester/tester.py:72,75-76 ---- */

/* A device image [H][W][channels] of 8-bit samples (channels 1, 3 or 4: PNG colour types 0, 2, 6) or [H][W] of 16-bit samples
 * (little-endian in memory, written big-endian) becomes the payload of one IDAT chunk minus its zlib wrapper: a sequence of deflate
 * blocks, one dynamic-Huffman block of literals (no matches) + one empty stored block per band of PF_PNG_BAND_ROWS rows, all non-final.
 * The caller adds the zlib header, a final empty stored block, the Adler-32 and the PNG chunks (postprocess.encode_png).  bgr != 0
 * (channels 3 or 4) swaps channels 0 and 2 on read.  Other channels / bits combinations, bgr with one channel and rows of more than
 * 2^28 - 1 bytes: PF_ERR_ARG.  Four steps:
 *   1. pf_png_workspace_bytes: sizes of the device workspace and of the output buffer, and the number of bands.
 *   2. pf_png_filter_histogram: picks each row's filter (None, Sub, Up or Paeth: smallest sum of |residual as int8|; kept in the
 *      workspace) and fills hist257 (device, 257 counts: the bytes of the filtered stream, filter bytes included, [256] = number of bands).
 *   3. pf_png_build_table: HOST ONLY, host pointers, no GPU call: hist257 -> table, PF_PNG_TABLE_WORDS words: [s] for s < 257 =
 *      bit-reversed canonical Huffman code | length << 16 (1 .. 15, 0 = unused), [257] = bits of the block header, [260 ..] = the header
 *      (BFINAL = 0, BTYPE = 2, HLIT = 0, HDIST = 0 with one distance code of length 0, HCLEN, code-length code, run symbols), at most 256 bytes.
 *   4. pf_png_encode: table on the device (8-byte aligned), same image arguments and workspace as step 2.  out receives the bands back
 *      to back; meta (device, 2 + 3 * nbands words) = total bytes (low, high), then per band {bytes, S1, S2} with S1 = sum of the band's
 *      stream bytes and S2 = sum of (n - i) * byte i over its n bytes, both mod 65521 (the Adler-32 partial sums).
 * workspace must be 16-byte aligned; its contents carry from step 2 to step 4. */
#define PF_PNG_BAND_ROWS 8
#define PF_PNG_TABLE_WORDS 324
int pf_png_workspace_bytes(int H, int W, int channels, int bits, long* workspace_bytes, long* out_bytes, int* nbands);
int pf_png_filter_histogram(const void* img, int H, int W, int channels, int bits, int bgr, void* workspace, uint32_t* hist257, void* stream);
int pf_png_build_table(const uint32_t* hist257, uint32_t* table);
int pf_png_encode(const void* img, int H, int W, int channels, int bits, int bgr, const uint32_t* table, void* workspace, uint8_t* out,
                  uint32_t* meta, void* stream);

/* ---- run matches for the same two files (csrc/png_rle.hip, csrc/png_huff.h): estimator/tester/tester.py:66-76 ---- */

/* The same images, bands, meta and container as above, with every run of equal bytes inside a row of the filtered stream coded as
 * deflate matches at distance 1 (zlib's Z_RLE): the first byte of a run is a literal, the rest is cut into chunks of 258, a chunk of
 * 3 or more bytes is one match, a trailing chunk of 1 or 2 bytes is literals.  Pays on the colour image, loses on the 16-bit one, so
 * step 2 counts for both codings at once and the caller chooses (postprocess.encode_png, strategy = 'huffman' | 'rle' | 'auto').
 *   1. pf_png_rle_workspace_bytes: as pf_png_workspace_bytes, sized for the larger slot of the two codings: the workspace and the
 *      output buffer serve pf_png_encode as well as pf_png_rle_encode.
 *   2. pf_png_rle_filter_histogram: pf_png_filter_histogram's filter choice; hist (device, 8-byte aligned, PF_PNG_RLE_HIST_WORDS
 *      words): [0 .. 256] the literal histogram pf_png_filter_histogram gives, [257 .. 542] the 286 token counts under the rule above
 *      (literals, [257 + 256] = number of bands, then matches by length symbol 257 .. 285), [543] zero, [544 .. 545] the total of the
 *      matches' extra bits (64 bits, low word first).
 *   3. pf_png_rle_build_table: HOST ONLY: the 286 token counts -> table, PF_PNG_RLE_TABLE_WORDS words: [s] for s < 286 = bit-reversed
 *      code | length << 16 (1 .. 14, 0 = unused), [286] = bits of the block header, [287] = the distance code (0 | 1 << 16),
 *      [288 + k] = base length | extra bits << 16 of length symbol 257 + k, [320 ..] = the header (HLIT <= 29, HDIST = 0 with one
 *      distance code of length 1), at most 272 bytes.
 *   4. pf_png_rle_encode: as pf_png_encode, with the table of step 3. */
#define PF_PNG_RLE_TABLE_WORDS 388
#define PF_PNG_RLE_HIST_WORDS 546
int pf_png_rle_workspace_bytes(int H, int W, int channels, int bits, long* workspace_bytes, long* out_bytes, int* nbands);
int pf_png_rle_filter_histogram(const void* img, int H, int W, int channels, int bits, int bgr, void* workspace, uint32_t* hist,
                                void* stream);
int pf_png_rle_build_table(const uint32_t* hist286, uint32_t* table);
int pf_png_rle_encode(const void* img, int H, int W, int channels, int bits, int bgr, const uint32_t* table, void* workspace,
                      uint8_t* out, uint32_t* meta, void* stream);

/* ---- JPEG decoding of the input image (csrc/jpeg.hip, csrc/jpeg_host.h): estimator/datasets/general_dataset.py:27,40 ---- */

/* A baseline JPEG file (SOF0, or SOF1 at 8 bits; one interleaved Huffman scan; grey, or YCbCr at 4:4:4, 4:2:2 or 4:2:0; optional restart
 * intervals) becomes a device image uint8 [H'][W'][3], RGB, bit-exact with libjpeg's defaults (islow inverse DCT, fancy upsampling).
 * Between the two halves lies the coefficient array: int16 [nblocks][64], natural (de-zigzagged) order, not dequantised, blocks in MCU
 * order and in scan order inside an MCU, DC absolute.  Both entropy paths (steps 3 and 6) fill it identically.  Steps:
 *   1. pf_jpeg_parse: HOST ONLY.  Markers up to the scan -> header.  Every refusal has its own PF_JPEG_E_* code.
 *   2. pf_jpeg_prepare_scan: HOST ONLY.  scan (capacity >= len - header.scan_begin + 68) receives the entropy-coded bytes with FF 00 ->
 *      FF and the RSTn markers removed, zero-padded by >= 64 bytes to a multiple of 4 (*scan_bytes, padding included); segs = {first
 *      bit, end bit} of each of the header.nsegments restart intervals.  Missing EOI, a foreign marker, RSTn out of sequence or count: error.
 *   3. pf_jpeg_decode_entropy_host: HOST ONLY.  The sequential entropy decoder: scan + segs -> coef (host).  The exact comparator of step 6.
 *   4. pf_jpeg_plan: HOST ONLY.  Cuts every segment into subsequences ("lanes") of subsequence_bits (a multiple of 32, 32 .. 2^20); lanes
 *      (null = count only; 3 words per lane: start bit, end bit, segment), segx (4 words per segment: end bit, first lane, first block,
 *      blocks), *nlanes, *longest = the most lanes one segment has.  pf_jpeg_build_tables: HOST ONLY, header -> PF_JPEG_TABLE_WORDS words.
 *   5. pf_jpeg_workspace_bytes: the device workspaces of steps 6 and 7.
 *   6. pf_jpeg_decode_entropy: scan, lanes, segx, tables, workspace and coef on the device (workspace and coef 16-byte aligned, scan 4-byte).
 *      Decodes every lane from a guessed state, re-decodes from the neighbour's exit state until a round changes nothing (*sync_rounds
 *      rounds; more than max_sync_rounds needed: PF_JPEG_NOT_CONVERGED, nothing usable in coef), writes the coefficients and makes the DCs
 *      absolute.  Synchronises the stream once per round (a launch, a 4-byte copy back and a wait) and once at the end.  A broken stream:
 *      PF_JPEG_E_STREAM.  PF_JPEG_NOT_CONVERGED returns without a final synchronise: kernels of the rounds so far may still be queued, so
 *      scan, lanes, segx, tables, workspace and coef must be released in stream order (as torch's caching allocator does) or after a
 *      synchronise.
 *   7. pf_jpeg_reconstruct: coef (device) -> rgb (device, H x W x 3, or W x H x 3 for orientations 5 .. 8): dequantisation, inverse DCT,
 *      upsampling, colour transform; the EXIF orientation (1 .. 8; pass 1 to ignore it) is applied in the store address. */
#define PF_JPEG_TABLE_WORDS 2152
#define PF_JPEG_E_NOT_JPEG 32
#define PF_JPEG_E_TRUNCATED 33
#define PF_JPEG_E_PROGRESSIVE 34
#define PF_JPEG_E_ARITHMETIC 35
#define PF_JPEG_E_LOSSLESS 36
#define PF_JPEG_E_PRECISION 37    /* 12-bit samples */
#define PF_JPEG_E_QUANT16 38      /* 16-bit quantisation table */
#define PF_JPEG_E_COMPONENTS 39   /* not 1 or 3 components */
#define PF_JPEG_E_COLORSPACE 40   /* Adobe transform other than YCbCr, or RGB component ids */
#define PF_JPEG_E_SAMPLING 41
#define PF_JPEG_E_MULTISCAN 42
#define PF_JPEG_E_DNL 43          /* DNL marker, or a height of 0 */
#define PF_JPEG_E_MARKER 44       /* a marker where none may stand */
#define PF_JPEG_E_RESTART 45      /* RSTn out of sequence or count */
#define PF_JPEG_E_NO_EOI 46
#define PF_JPEG_E_TABLE 47        /* missing or invalid Huffman / quantisation table */
#define PF_JPEG_E_STREAM 48       /* entropy-coded data does not decode to the frame */
#define PF_JPEG_E_SCAN 49         /* scan header other than one full sequential scan */
#define PF_JPEG_NOT_CONVERGED 64
struct pf_jpeg_header {
  int32_t width, height, ncomp, hmax, vmax;
  int32_t restart_interval;       /* MCUs, 0 = none */
  int32_t orientation;            /* EXIF 1..8 (1 when absent or out of range) */
  int32_t scan_begin;             /* byte offset of the first entropy-coded byte */
  int32_t mcus_x, mcus_y, blocks_per_mcu, nblocks, nsegments;
  int32_t sof;                    /* 0 (SOF0) or 1 (SOF1); 2 (SOF2) from pf_jpeg_prog_parse */
  int32_t comp_id[4], comp_h[4], comp_v[4], comp_tq[4], comp_td[4], comp_ta[4];   /* h, v as decoded (1 x 1 for a single component) */
  uint8_t qt[4][64];              /* natural order */
  uint8_t qt_present[4];
  uint8_t huff_bits[8][17];       /* [class * 4 + id][code length], class 0 = DC, 1 = AC */
  uint8_t huff_vals[8][256];
  uint8_t huff_present[8];
};
typedef struct pf_jpeg_header pf_jpeg_header;
int pf_jpeg_parse(const uint8_t* data, long len, pf_jpeg_header* header);
int pf_jpeg_prepare_scan(const uint8_t* data, long len, const pf_jpeg_header* header, uint8_t* scan, long scan_capacity, long* scan_bytes,
                         uint32_t* segs);
int pf_jpeg_decode_entropy_host(const pf_jpeg_header* header, const uint8_t* scan, long scan_bytes, const uint32_t* segs, int16_t* coef);
int pf_jpeg_plan(const pf_jpeg_header* header, const uint32_t* segs, int subsequence_bits, uint32_t* lanes, long lane_capacity,
                 uint32_t* segx, int* nlanes, int* longest);
int pf_jpeg_build_tables(const pf_jpeg_header* header, uint32_t* tables);
int pf_jpeg_workspace_bytes(const pf_jpeg_header* header, int nlanes, long* entropy_bytes, long* recon_bytes);
int pf_jpeg_decode_entropy(const pf_jpeg_header* header, const uint8_t* scan, long scan_bytes, const uint32_t* lanes, const uint32_t* segx,
                           int nlanes, int longest, const uint32_t* tables, int max_sync_rounds, void* workspace, int16_t* coef,
                           int* sync_rounds, void* stream);
int pf_jpeg_reconstruct(const pf_jpeg_header* header, const int16_t* coef, int orientation, void* workspace, uint8_t* rgb, void* stream);

/* ---- progressive JPEG, opt-in (csrc/jpeg_prog.hip, csrc/jpeg_host.h) ----
 * A progressive file (SOF2, 8 bits, Huffman; colour, sampling and orientation rules as above) fills the same coefficient array, scan by
 * scan, and is then reconstructed by pf_jpeg_reconstruct.  Only complete progressions are accepted (every coefficient of every component
 * refined down to bit 0): libjpeg smooths the blocks of an incomplete one.  A scan is interleaved with every component in frame order (DC
 * scans only), or holds one component; a one-component scan walks that component's own ceil(wc / 8) x ceil(hc / 8) blocks in raster order
 * (wc = ceil(W * h / hmax)), its restart intervals count those blocks, and a block map turns its block order into the array's MCU order.
 * Steps, all names carrying the prefix pf_jpeg_prog_:
 *   1. _parse: HOST ONLY.  The whole file -> the frame header (restart_interval 0, nsegments 1: restart intervals belong to scans) and the
 *      scan list (capacity: the number of FF DA byte pairs in the file is enough): kind, components, band, Ah, Al, the Huffman tables as
 *      they stand at that SOS, the byte range of its entropy-coded data and its restart interval.  Progression bookkeeping as libjpeg's
 *      coef_bits; every refusal has its own PF_JPEG_E_PROG_* code.  A baseline file: PF_JPEG_PROG_BASELINE, nothing else done.
 *   2. _prepare_scan: HOST ONLY.  As pf_jpeg_prepare_scan for one scan (capacity >= end - begin + 68); segs = scan.nsegments pairs.
 *   3. _decode_scan_host: HOST ONLY.  The sequential decoder of jdphuff.c for one scan of any kind, applied to coef (host, zeroed by the
 *      caller before the first scan).  The second entropy path and the exact comparator of steps 6 to 8.
 *   4. _refine_ac_host: HOST ONLY.  An AC-refinement scan decoded against the non-zero masks of its component's blocks (one uint64 per
 *      block of the scan, bit k = the coefficient at zigzag position k is non-zero) -> records, three uint64 per block {correction, new, sign of
 *      new} in the same bit order, and the masks updated.  AC refinement is not self-synchronising, so it has no device decoder.
 *   5. _plan, _build_tables, _block_map, _workspace_bytes: HOST ONLY.  The subsequence plan and decode tables of one scan (layouts as
 *      pf_jpeg_plan and pf_jpeg_build_tables; slot 2 * i = DC table of the scan's component i, slot 1 = its AC table), the block map of a
 *      one-component scan (int32 per block of the scan), and the device workspace of step 6.
 *   6. _decode_scan: a DC-first or AC-first scan on the device, in the manner of pf_jpeg_decode_entropy (same arguments, status codes and
 *      synchronisation; map = null for an interleaved scan).  coef is NOT zeroed: the caller zeroes it once before the first scan.
 *   7. _dc_refine: a DC-refinement scan, one thread per block (segs on the device).
 *   8. _nonzero_mask: coef -> the masks of step 4 for one component; _apply_refinement: the records of step 4 -> coef. */
#define PF_JPEG_E_PROG_NO_FIRST 50       /* refinement of a coefficient that had no first scan */
#define PF_JPEG_E_PROG_AH 51             /* Ah is not the Al of the scan before (or a first scan comes twice) */
#define PF_JPEG_E_PROG_AL 52             /* a refinement with Al != Ah - 1 */
#define PF_JPEG_E_PROG_AC_COMPONENTS 53  /* AC scan with more than one component */
#define PF_JPEG_E_PROG_AC_BEFORE_DC 54   /* AC scan before its component's DC */
#define PF_JPEG_E_PROG_BAND 55           /* Ss > Se, Se > 63, or a DC scan with Se != 0 */
#define PF_JPEG_E_PROG_INCOMPLETE 56     /* some coefficient never sent or not refined to bit 0: libjpeg would smooth the file */
#define PF_JPEG_PROG_BASELINE 65         /* not an error: the file is baseline, use pf_jpeg_parse */
#define PF_JPEG_PROG_DC_FIRST 0
#define PF_JPEG_PROG_DC_REFINE 1
#define PF_JPEG_PROG_AC_FIRST 2
#define PF_JPEG_PROG_AC_REFINE 3
struct pf_jpeg_prog_scan {
  int32_t kind;                   /* PF_JPEG_PROG_DC_FIRST .. PF_JPEG_PROG_AC_REFINE */
  int32_t ncomp, comp[4];         /* indices into the frame's components, in frame order */
  int32_t td[4], ta[4];
  int32_t ss, se, ah, al;
  int32_t restart_interval;       /* in units of this scan: MCUs when interleaved, blocks otherwise; 0 = none */
  int32_t begin, end;             /* the scan's entropy-coded bytes in the file: [begin, end), end = the next marker that is not RSTn */
  int32_t blocks_per_unit, nblocks, nsegments;    /* the scan's own walk */
  int32_t blocks_x, blocks_y;     /* one-component scan: the component's blocks across and down */
  uint8_t huff_bits[8][17];       /* the tables as they stand at this SOS, laid out as in pf_jpeg_header */
  uint8_t huff_vals[8][256];
};
typedef struct pf_jpeg_prog_scan pf_jpeg_prog_scan;
int pf_jpeg_prog_parse(const uint8_t* data, long len, pf_jpeg_header* header, pf_jpeg_prog_scan* scans, int scan_capacity, int* nscans);
int pf_jpeg_prog_prepare_scan(const uint8_t* data, long len, const pf_jpeg_prog_scan* scan, uint8_t* out, long capacity, long* scan_bytes,
                              uint32_t* segs);
int pf_jpeg_prog_decode_scan_host(const pf_jpeg_header* header, const pf_jpeg_prog_scan* scan, const uint8_t* bytes, long scan_bytes,
                                  const uint32_t* segs, int16_t* coef);
int pf_jpeg_prog_refine_ac_host(const pf_jpeg_prog_scan* scan, const uint8_t* bytes, long scan_bytes, const uint32_t* segs, uint64_t* masks,
                                uint64_t* records);
int pf_jpeg_prog_plan(const pf_jpeg_prog_scan* scan, const uint32_t* segs, int subsequence_bits, uint32_t* lanes, long lane_capacity,
                      uint32_t* segx, int* nlanes, int* longest);
int pf_jpeg_prog_build_tables(const pf_jpeg_prog_scan* scan, uint32_t* tables);
int pf_jpeg_prog_block_map(const pf_jpeg_header* header, const pf_jpeg_prog_scan* scan, int32_t* map);
int pf_jpeg_prog_workspace_bytes(int nlanes, int scan_blocks, long* bytes);
int pf_jpeg_prog_decode_scan(const pf_jpeg_header* header, const pf_jpeg_prog_scan* scan, const uint8_t* bytes, long scan_bytes,
                             const uint32_t* lanes, const uint32_t* segx, int nlanes, int longest, const uint32_t* tables,
                             const int32_t* map, int max_sync_rounds, void* workspace, int16_t* coef, int* sync_rounds, void* stream);
int pf_jpeg_prog_dc_refine(const pf_jpeg_header* header, const pf_jpeg_prog_scan* scan, const uint8_t* bytes, long scan_bytes,
                           const uint32_t* segs, const int32_t* map, int16_t* coef, void* stream);
int pf_jpeg_prog_nonzero_mask(const pf_jpeg_header* header, const pf_jpeg_prog_scan* scan, const int16_t* coef, const int32_t* map,
                              uint64_t* masks, void* stream);
int pf_jpeg_prog_apply_refinement(const pf_jpeg_header* header, const pf_jpeg_prog_scan* scan, const uint64_t* records, const int32_t* map,
                                  int16_t* coef, void* stream);

/* ---------------------------------------------------------------- PNG decoding of the input image (csrc/png_decode.hip, csrc/png_host.h,
 * csrc/png_inflate.h).  Non-interlaced files of every colour type and bit depth; the inflate runs on the device:
 *   1. pf_pngd_parse: HOST ONLY.  Chunk walk, IHDR / PLTE / tRNS validation, the IDAT payloads concatenated behind the zlib header
 *      (which is checked) into `deflate`.  Every refusal has its own PF_PNGD_E_* code.
 *      The device (and *_host) steps take the deflate data as little-endian 32-bit `words` with PF_PNGD_PAD_WORDS zero words behind.
 *   2. pf_pngd_find: one thread per bit offset tests for a well-formed dynamic block header and appends the offset to `list`
 *      (capacity words); *count keeps counting past the capacity, nothing is written past it.  Offset 0 is listed when a fixed or
 *      dynamic block starts there.
 *   3. pf_pngd_scan: one wave per listed start decodes to the end-of-block code without storing; records of four words
 *      {start bit, end bit, output bytes, status | BFINAL << 8}, status one of PF_PNGD_S_*.
 *   4. the chain walk is the caller's (preprocess.decode_png): it yields the block table, four words per block
 *      {start (bit of the header; byte of the data for a stored block), type, output offset, output bytes}.
 *   5. pf_pngd_inflate: one wave per block writes literals to `lit` and a 32-bit reference per output byte to `ref`.
 *   6. pf_pngd_resolve: `rounds` pointer-jumping launches, then the gather into `out`.
 *   7. pf_pngd_unfilter: `inflated` (height rows of 1 + rowbytes) -> `recon` (height rows of rowbytes), exact per the specification.
 *   8. pf_pngd_expand: `recon` -> the image for the cases whose layout differs from it (sub-byte samples, palette, 16-bit byte order).
 *   9. pf_pngd_adler: the Adler-32 of `data` into result[0].
 * `status` (a device word, zeroed by the caller) collects PF_PNGD_F_* flags from steps 5, 7 and 8.  Every device step is ordered on
 * `stream`; none synchronises.  pf_pngd_find_host, pf_pngd_scan_host and pf_pngd_inflate_model_host are the same code run
 * sequentially on the host (no GPU call), for tests.
 * pf_pngd_to_rgb8: any decoded layout -> uint8 [H,W,3]: grey replicated, alpha dropped, 16-bit samples keep their high byte. */
#define PF_PNGD_E_SIGNATURE 80
#define PF_PNGD_E_CHUNK 81        /* chunk length, a truncated file, an unknown critical chunk, a bad tRNS */
#define PF_PNGD_E_ORDER 82        /* chunk order */
#define PF_PNGD_E_CRC 83          /* CRC of a critical chunk other than IDAT */
#define PF_PNGD_E_IHDR 84         /* a combination the specification forbids */
#define PF_PNGD_E_INTERLACED 85   /* Adam7 */
#define PF_PNGD_E_ZLIB 86         /* zlib header: CM != 8, window > 32 KiB, FDICT, FCHECK */
#define PF_PNGD_E_STREAM 87       /* invalid or truncated deflate stream */
#define PF_PNGD_E_DISTANCE 88     /* a match reaches before the start of the output */
#define PF_PNGD_E_SIZE 89         /* inflated size != height * (1 + rowbytes) */
#define PF_PNGD_E_ADLER 90
#define PF_PNGD_E_FILTER 91       /* a row's filter type is above 4 */
#define PF_PNGD_E_PLTE 92         /* missing or invalid PLTE, or a pixel indexes past it */
#define PF_PNGD_E_IDAT_CRC 93     /* only with check_idat_crc */
#define PF_PNGD_PAD_WORDS 2       /* zero words the caller puts behind the deflate data: `words` holds (nbits + 31) / 32 + 2 (nwords says so) */
#define PF_PNGD_S_OK 0
#define PF_PNGD_S_INVALID 1
#define PF_PNGD_S_LIMIT 2         /* max_block_bits reached */
#define PF_PNGD_S_EOS 3           /* end of the stream reached */
#define PF_PNGD_S_SIZE 4          /* more output than the image holds */
#define PF_PNGD_S_DIST 5
#define PF_PNGD_F_STREAM 1
#define PF_PNGD_F_DISTANCE 2
#define PF_PNGD_F_FILTER 4
#define PF_PNGD_F_PLTE 8
struct pf_pngd_header {
  int32_t width, height, depth, color_type, interlace;
  int32_t channels, bpp;          /* bpp = max(1, channels * depth / 8): the filters' byte distance */
  int32_t has_trns, plte_entries, idat_chunks;
  int64_t rowbytes, inflated_bytes, compressed_bytes;   /* inflated_bytes = height * (1 + rowbytes); compressed = the IDAT payloads */
  uint8_t palette[768];
};
typedef struct pf_pngd_header pf_pngd_header;
int pf_pngd_parse(const uint8_t* data, long len, int check_idat_crc, pf_pngd_header* header, uint8_t* deflate, long capacity, long* deflate_len);
int pf_pngd_find_host(const uint32_t* words, long nwords, uint32_t nbits, uint32_t* list, long capacity, long* count);
int pf_pngd_scan_host(const uint32_t* words, long nwords, uint32_t nbits, const uint32_t* starts, int n, uint32_t max_block_bits, uint32_t expected,
                      uint32_t* records);
int pf_pngd_inflate_model_host(const uint8_t* deflate, long len, long expected, uint32_t max_block_bits, uint8_t* out, long* stats);
int pf_pngd_find(const uint32_t* words, long nwords, uint32_t nbits, uint32_t* list, uint32_t capacity, uint32_t* count, void* stream);
int pf_pngd_scan(const uint32_t* words, long nwords, uint32_t nbits, const uint32_t* starts, int n, uint32_t max_block_bits, uint32_t expected,
                 uint32_t* records, void* stream);
int pf_pngd_inflate(const uint32_t* words, long nwords, uint32_t nbits, const uint32_t* blocks, int nblocks, uint32_t expected, uint8_t* lit,
                    uint32_t* ref, uint32_t* status, void* stream);
int pf_pngd_resolve(const uint8_t* lit, uint32_t* ref, uint32_t n, int rounds, uint8_t* out, void* stream);
int pf_pngd_unfilter(const uint8_t* inflated, const pf_pngd_header* header, uint8_t* recon, uint32_t* status, void* stream);
int pf_pngd_expand(const uint8_t* recon, const pf_pngd_header* header, const uint8_t* palette, void* image, uint32_t* status, void* stream);
int pf_pngd_adler(const uint8_t* data, long n, uint64_t* sums, uint32_t* result, void* stream);
int pf_pngd_to_rgb8(const void* image, int height, int width, int channels, int bits, uint8_t* rgb, void* stream);
/* Steps 3 and 5 with the symbols of a block decoded in parallel subsequences (csrc/png_inflate_par.hip; the scheme is stated in
 * csrc/png_inflate.h): one workgroup of pf_pngd_par_window() threads per candidate / per block, every thread one lane of
 * `subsequence_bits` bits (a multiple of 32 in 64 .. 65536).  The arguments and their checks are those of pf_pngd_scan / pf_pngd_inflate;
 * the records are the same wherever pf_pngd_scan's status is PF_PNGD_S_OK and carry some other status elsewhere; after
 * pf_pngd_inflate_par a reference points to a literal or into a strictly earlier lane's range, so pf_pngd_resolve needs
 * ceil(log2(lane ranges + stored blocks)) + 1 rounds.  `max_rounds` (a device word, zeroed by the caller) is raised to the largest number
 * of rounds a window needed.  The *_host entries run the same lane decoder through the same round schedule in plain loops on host
 * pointers (no GPU call), for tests. */
int pf_pngd_par_window(void);
int pf_pngd_scan_par_host(const uint32_t* words, long nwords, uint32_t nbits, const uint32_t* starts, int n, uint32_t max_block_bits, uint32_t expected,
                          uint32_t subsequence_bits, uint32_t* records, uint32_t* max_rounds);
int pf_pngd_inflate_par_host(const uint32_t* words, long nwords, uint32_t nbits, const uint32_t* blocks, int nblocks, uint32_t expected,
                             uint32_t subsequence_bits, uint8_t* lit, uint32_t* ref, uint32_t* status, uint32_t* max_rounds);
int pf_pngd_scan_par(const uint32_t* words, long nwords, uint32_t nbits, const uint32_t* starts, int n, uint32_t max_block_bits, uint32_t expected,
                     uint32_t subsequence_bits, uint32_t* records, uint32_t* max_rounds, void* stream);
int pf_pngd_inflate_par(const uint32_t* words, long nwords, uint32_t nbits, const uint32_t* blocks, int nblocks, uint32_t expected,
                        uint32_t subsequence_bits, uint8_t* lit, uint32_t* ref, uint32_t* status, uint32_t* max_rounds, void* stream);

/* ---------------------------------------------------------------- ground-truth depth files of the evaluation loop (csrc/gtread.hip):
 * estimator/datasets/general_dataset.py:60-143 (DepthMap) and u4k_dataset.py:118-119,168.  `src` is the PAYLOAD of the file as it lies
 * on disk, uploaded from the payload's offset (so it starts at the first sample, aligned to the sample's size; 16-byte alignment selects
 * the wide loads), or the uint8 / uint16 image pf_pngd_expand made.  One launch writes depth [H][W] float32 and, when edge_src is not
 * null, the plane the reference passes to get_boundaries (feed it to pf_depth_boundaries).  x = float32(sample); a and b are float32
 * constants the HOST has rounded the way numpy rounds a Python float that meets a float32 array; every +, - and / is one correctly
 * rounded float32 operation, denormals kept:
 *   mode                kinds              depth                                                     edge source            a, b
 *   PF_GT_U4K           F16 F32 F64        a / x                                                     x                      depth factor, -
 *   PF_GT_MID           F32                (a / (x + b)) / 1000, then 0 where x == +inf              x with +inf -> 0       f * baseline, doffs
 *   PF_GT_ETH3D         F32 (no swap)      x with NaN, +inf, -inf -> 0                               = depth                -, -
 *   PF_GT_GTA           U8 U16             x / 256                                                   = depth                -, -
 *   PF_GT_CITYSCAPES    U8 U16             d = x > 0 ? (x - 1) / 256 : 0;  a / d, NaN, +-inf -> 0    = depth                0.209313 * 2262.52, -
 *   PF_GT_RAW           F16 F32 F64        x (read_pfm, read_npy; W = width * 3 for a colour PFM)    = depth                -, -
 * Only +inf is masked in PF_GT_MID: -inf and NaN come out as the arithmetic gives them (-0.0 and NaN), as in the reference.
 * flags: PF_GT_SWAP = the samples are big-endian (float kinds only), PF_GT_FLIP = output row y reads source row H - 1 - y (PFM stores
 * the bottom row first).  Refused (PF_ERR_ARG): null src or depth, H or W <= 0, H * W >= 2^31, an unknown kind, mode or flag, a kind /
 * mode / swap combination the table does not have, src not aligned to its sample, depth or edge_src not 16-byte aligned.  src must hold
 * H * W samples; no plane may overlap another. */
#define PF_GT_F16 0
#define PF_GT_F32 1
#define PF_GT_F64 2
#define PF_GT_U8 3
#define PF_GT_U16 4
#define PF_GT_U4K 0
#define PF_GT_MID 1
#define PF_GT_ETH3D 2
#define PF_GT_GTA 3
#define PF_GT_CITYSCAPES 4
#define PF_GT_RAW 5
#define PF_GT_SWAP 1
#define PF_GT_FLIP 2
int pf_gt_convert(const void* src, int kind, int flags, int mode, int H, int W, float a, float b, float* depth, float* edge_src, void* stream);

/* ---------------------------------------------------------------- training-side augmentations of UnrealStereo4kDataset (csrc/augment.hip):
 * estimator/datasets/u4k_dataset.py:121-134 with transformers/augmentations.py (aug_rotate, aug_color, aug_flip).  The HOST draws every
 * random number and builds the matrix; both entry points are pure functions of their arguments.  m and colour (and a below) are HOST
 * arrays, read before the call returns.
 *
 * pf_aug_image_u8_to_f32: img uint8 [H][W][3] in the raw file's order (B, G, R) -> out float32 [3][H][W] (R, G, B).  Output (y, x)
 * is Image.rotate(angle, resample=BILINEAR) of Pillow at (flip ? W - 1 - x : x, y), bit for bit: with m[6] the matrix Image.rotate
 * builds (angle % 360, a = -radians(angle), cos and sin rounded to 15 decimals, centre (W/2, H/2)), in double and without contraction
 *   xs = m0 (x + 0.5) + m1 (y + 0.5) + m2,  ys = m3 (x + 0.5) + m4 (y + 0.5) + m5;  0 if xs < 0 || xs >= W || ys < 0 || ys >= H;
 *   xin = xs - 0.5, x0 = floor(xin), dx = xin - x0 (the same in y); columns x0 and x0 + 1 clamped to [0, W - 1], row y0 clamped, row
 *   y0 + 1 only if inside the image (else v2 = v1); every blend a + (b - a) d, along x then along y; truncated to a byte.
 * Then numpy's float32 arithmetic: v = float32(byte) / 255.0f and, if colour_on,
 *   v = float32(pow(double(v), double(gamma)));  v = v * brightness;  v = float32(double(v) * colour[c]);  v = min(max(v, 0), 1)
 * with gamma and brightness already rounded to float32 by the host and colour[c] indexed by the OUTPUT channel (R, G, B).  numpy's
 * float32 `**` differs from the correctly rounded power in its last bit at some operands, so with colour_on the result is within one
 * float32 rounding per step of the exact chain rather than equal to numpy's; without it the plane equals the reference bit for bit.
 * Refused (PF_ERR_ARG): null img, out or m (or colour with colour_on), H or W <= 0, H * W >= 2^31, a matrix entry that is not finite,
 * out not 16-byte aligned, img and out overlapping.
 *
 * pf_aug_planes_nearest: src0 (and src1, or null with dst1 null) float32 [H][W] -> dst0 (dst1): Image.rotate(angle, resample=NEAREST)
 * on a mode 'F' image, Pillow's 16.16 fixed-point path, then the flip.  a[6] = FIX(m0), FIX(m1), FIX(m2 + m0 / 2 + m1 / 2), FIX(m3),
 * FIX(m4), FIX(m5 + m3 / 2 + m4 / 2) with FIX(v) = floor(v * 65536 + 0.5); for x' = flip ? W - 1 - x : x the source is
 *   sx = (a2 + x' a0 + y a1) >> 16,  sy = (a5 + x' a3 + y a4) >> 16   (64-bit sums, arithmetic shift)
 * and the output is 0 where (sx, sy) is outside the plane -- for the depth plane too (not factor / 0).
 * Refused (PF_ERR_ARG): null src0, dst0 or a, exactly one of src1 / dst1 null, H or W <= 0, H * W >= 2^31, a destination not 16-byte
 * aligned, any two of the planes overlapping. */
int pf_aug_image_u8_to_f32(const unsigned char* img, int H, int W, const double* m, int flip, int colour_on, float gamma, float brightness,
                           const double* colour, float* out, void* stream);
int pf_aug_planes_nearest(const float* src0, const float* src1, int H, int W, const int* a, int flip, float* dst0, float* dst1, void* stream);

/* ---- backward of the metric-bins head and of the SILog loss (csrc/head_bwd.hip) ----
 * All tensors float32, NHWC with a pixel stride (ld) like the forward's.  No entry point uses a float atomic: every sum has a fixed order, two
 * calls on the same operands give the same bits.  Every call refuses (PF_ERR_ARG, before any launch) a null or misaligned pointer (4 bytes for
 * float, 8 for double), a size below 1 and a pixel stride below the channel count.
 *
 * pf_conv1x1_wgrad: dw[N][K] = sum_p dy[p][n] x[p][k] and (db not null) db[N] = sum_p dy[p][n] over P pixels, on the float32 MFMA
 *   (v_mfma_f32_16x16x4_f32).  P is split into blocks of rows_per_block pixels (0: the default, about 512 blocks and never fewer than 512
 *   pixels each); every block writes a partial [N][K] tile and a partial [N] to the workspace, a second launch adds them in block order.
 *   pf_conv1x1_wgrad_workspace_bytes gives the workspace size for the same (P, N, K, rows_per_block); N, K <= 4096, at most 65535 blocks.
 * pf_resize_bilinear_bwd: the adjoint of the align_corners=True bilinear resize [B,H,W,C] -> [B,OH,OW,C]: dx[B,H,W,C] (+)= up^T(dy[B,OH,OW,C]),
 *   a gather over the destination pixels whose footprint holds the source pixel, with the forward's own weights; accumulate != 0 adds to dx.
 * pf_attractor_bwd: AttractorLayerUnnormed.  With c = up(b_prev) [B,h,w,n_bins], dx = A_i - c_j, s = 1 / n_attr (kind 'mean') or 1 ('sum'),
 *   f' = (1 - 300 dx^2) / (1 + 300 dx^2)^2 ('inv') or exp(-300 dx^2) (1 - 600 dx^2) ('exp') and g = d_b_new:
 *   dA[B,h,w,i] = s sum_j g_j f'(dx),  d_b_c[B,h,w,j] = g_j (1 - s sum_i f'(dx)); the gradient of b_prev is pf_resize_bilinear_bwd of d_b_c.
 *   n_bins <= 256.
 * pf_logbinom_depth_bwd: pt [B,h,w,>=4] (after softplus), centers [B,hc,wc,n_bins], d_depth [B,h,w] -> d_pt [B,h,w,4] (stride d_pt_ld) and
 *   d_centers_up [B,h,w,n_bins] = probs * d_depth (its resize adjoint is the gradient of centers).  The softmax is recomputed; the two
 *   clamp(., 1e-4, 1) pass no gradient where they bind.  2 <= n_bins <= 256.  logc (device, n_bins floats, or null): log C(n_bins - 1, k) in the
 *   Stirling form of dist_layers.py:29-45 as the reference's float32 tensor arithmetic gives it.  These are constants of the model; at a
 *   temperature t a last-bit difference in one of them (1.5e-5 at values near 200) moves that bin's probability by 1.5e-5 / t, so a caller who
 *   wants the reference's gradient hands in the reference's constants.  Null: the same expression evaluated in the kernel.
 * pf_act_bwd: dy[p][c] *= act'; PF_ACT_RELU and PF_ACT_SOFTPLUS (1 - exp(-y)) take the layer's OUTPUT as ref, PF_ACT_GELU (exact erf form) the
 *   PRE-ACTIVATION.
 * pf_silog_loss_bwd: d_pred[n] = d_loss * dL/dpred from the three sums pf_silog_loss left in ws3 (count, sum g, sum g^2; unbiased variance);
 *   all zeros when at most one pixel is valid (and where the loss is exactly zero, whose derivative does not exist). */
int pf_conv1x1_wgrad_workspace_bytes(long P, int N, int K, int rows_per_block, long* bytes);
int pf_conv1x1_wgrad(const float* dy, int dy_ld, const float* x, int x_ld, long P, int N, int K, float* dw, float* db, void* workspace,
                     long workspace_bytes, int rows_per_block, void* stream);
int pf_resize_bilinear_bwd(const float* dy, int dy_ld, int B, int OH, int OW, int C, float* dx, int dx_ld, int H, int W, int accumulate,
                           void* stream);
int pf_attractor_bwd(const float* A, int a_ld, int n_attr, int attractor_exp, int kind_sum, const float* b_prev, int hp, int wp,
                     const float* d_b_new, float* dA, int da_ld, float* d_b_c, int B, int h, int w, int n_bins, void* stream);
int pf_logbinom_depth_bwd(const float* pt, int pt_ld, const float* centers, int hc, int wc, const float* d_depth, float* d_pt, int d_pt_ld,
                          float* d_centers_up, int B, int h, int w, int n_bins, float min_temp, float max_temp, const float* logc, void* stream);
int pf_act_bwd(float* dy, int dy_ld, const float* ref, int ref_ld, long P, int C, int act, void* stream);
int pf_silog_loss_bwd(const float* pred, const float* target, long n, float min_depth, float max_depth, float beta, const double* sums3,
                      float d_loss, float* d_pred, void* stream);

#ifdef __cplusplus
}
#endif
#endif
