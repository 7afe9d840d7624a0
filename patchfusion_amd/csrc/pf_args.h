// Host side of the C ABI: the argument checks that the launchers share.  Every launcher refuses (PF_ERR_ARG) what its kernels cannot address BEFORE
// anything is launched; include/pf_hip.h states the refusals per entry point and tests/envelope.py lists them row by row.
#pragma once
#include <stdint.h>
#include "pf_common.h"
#include "../../include/pf_hip.h"

// the text behind pf_last_error(): "<entry point>: <reason>" (csrc/igemm.hip owns the thread-local buffer)
void pf_set_error(const char* fn, const char* why);
inline int pf_refuse(const char* fn, const char* why) {
  pf_set_error(fn, why);
  return PF_ERR_ARG;
}

inline bool pf_bad_dtype(int dtype) { return dtype != PF_DTYPE_F32 && dtype != PF_DTYPE_BF16; }
inline bool pf_bad_act(int act) { return act < PF_ACT_NONE || act > PF_ACT_SOFTPLUS; }

// sizes of a convolution described by pf_conv_params: everything positive and the output grid the one the input, the filter, the stride and the
// padding give (the kernels bound-check taps against H x W but index y by OH x OW)
inline const char* pf_conv_geometry(const pf_conv_params& p) {
  if (p.B <= 0 || p.H <= 0 || p.W <= 0 || p.OH <= 0 || p.OW <= 0) return "B, H, W, OH, OW must be positive";
  if (p.KH <= 0 || p.KW <= 0 || p.stride <= 0 || p.pad < 0) return "KH, KW, stride must be positive, pad >= 0";
  if (p.H + 2L * p.pad < p.KH || p.W + 2L * p.pad < p.KW) return "filter larger than the padded input";
  if ((p.H + 2L * p.pad - p.KH) / p.stride + 1 != p.OH || (p.W + 2L * p.pad - p.KW) / p.stride + 1 != p.OW)
    return "OH, OW must be (H + 2 pad - KH) / stride + 1, (W + 2 pad - KW) / stride + 1";
  return nullptr;
}

// the epilogue operands of a pf_conv_params (device side: csrc/pf_epilogue.h), each optional: bias / scale off a vec_align-byte boundary, res / res2
// off a res_align-byte one (the widest load the launcher's kernels issue through them), or a residual whose rows are not a multiple of 4 elements
// apart or closer than Cout
inline const char* pf_epilogue_operands(const pf_conv_params& p, unsigned vec_align, unsigned res_align) {
  if (pf_misaligned(p.bias, vec_align) || pf_misaligned(p.scale, vec_align)) return "misaligned bias / scale";
  if (pf_misaligned(p.res, res_align) || pf_misaligned(p.res2, res_align)) return "misaligned residual";
  if ((p.res && (p.res_ld % 4 || p.res_ld < p.Cout)) || (p.res2 && (p.res2_ld % 4 || p.res2_ld < p.Cout)))
    return "residual ld must be a multiple of 4 and at least Cout";
  return nullptr;
}

// a pf_conv_params used as a LINEAR layer (the split-precision, fp16x2 and bf16 ping-pong GEMMs): M = B * OH * OW rows, 1 x 1 / stride 1 / no
// padding / no pixel shuffle, a known activation, at most 65535 planes
inline const char* pf_linear_envelope(const pf_conv_params& p) {
  if (p.KH != 1 || p.KW != 1 || p.stride != 1 || p.pad != 0 || p.shuffle != 1) return "1x1 / stride 1 / pad 0 / shuffle 1 (linear layers) only";
  if (const char* e = pf_conv_geometry(p)) return e;
  if (pf_bad_act(p.act)) return "bad act";
  if (p.batch < 0 || p.batch > PF_GRID_YZ_MAX) return "batch must be in [0, 65535]";
  if (p.Cin <= 0 || p.Cout <= 0) return "Cin, Cout must be positive";
  return nullptr;
}

// the batched fp16x2 product of the transform points, on either tile (pf_gemm_f16x2_points, pf_gemm_f16x2_points128): PF_OK, or the refusal of `fn`
inline int f16x2_points_envelope(const char* fn, const pf_conv_params* p, const int* col_exp) {
  if (!p || !p->x || !p->w || !p->y || !col_exp) return pf_refuse(fn, "null tensor");
  if (const char* e = pf_linear_envelope(*p)) return pf_refuse(fn, e);
  if (pf_misaligned(p->x, 16) || pf_misaligned(p->w, 16) || pf_misaligned(p->y, 16) || pf_misaligned(col_exp, 16)) return pf_refuse(fn, "misaligned tensor");
  if (p->y_ld < p->Cout || p->x_bstride % 8 || p->w_bstride % 8 || (p->batch > 1 && p->y_bstride % 4)) return pf_refuse(fn, "y_ld below Cout or misaligning plane strides");
  const long M = (long)p->B * p->OH * p->OW;
  if (p->korder != 6 || !p->out_f32) return pf_refuse(fn, "korder must be 6, the output float32");
  if (p->Cin <= 0 || p->Cin % 32 || p->x_ld != p->Cin || p->Kpad != p->Cin || p->Cout <= 0 || p->Cout % 4 || p->y_ld % 4 || p->w_rows < p->Cout ||
      p->w_rows % 4 || M <= 0 || M * 64 >= (1L << 31) || (long)p->w_rows * 64 >= (1L << 31) || p->x_bstride <= 0 || p->w_bstride <= 0 || p->bias ||
      p->scale || p->res || p->res2 || p->act != PF_ACT_NONE || p->batch > 65535)
    return pf_refuse(fn, "argument outside the envelope (include/pf_hip.h)");
  return PF_OK;
}
