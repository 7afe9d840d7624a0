// The output epilogue that every kernel finishing a pf_conv_params layer shares:   y = (act(v + bias) * scale) + res + res2
// on the four consecutive output channels a lane holds.  The activation and the residual step live here once; a kernel keeps what is schedule
// (the order of its fragments, its sched_barriers, where it fetches bias / scale, its debug switches) around the calls.  Everything is forced
// inline.  These kernels are register-tight: a site takes a helper only where every kernel of its file still compiles to the instructions it
// had with the text written out (compare the device assembly against the parent commit when a helper or a call site changes).
#pragma once
#include "pf_common.h"
#include "../../include/pf_hip.h"

// act by its PF_ACT_* code (uniform per launch: one branch, then four independent chains)
__device__ __forceinline__ void epi_act(float (&v)[4], int act) {
  if (act == PF_ACT_RELU) {
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] = fmaxf(v[r], 0.f);
  } else if (act == PF_ACT_GELU) {
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] = gelu_erf(v[r]);
  } else if (act == PF_ACT_SOFTPLUS) {
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] = softplus20(v[r]);
  }
}

// + res[row][col .. col + 3] of an optional residual of element type R (float or bf16_t), leading dimension ld.  `ok` is the row / column
// predicate of the sites whose lanes run the epilogue unconditionally.  The address is formed INSIDE the null check, from (row, ld, col): an
// offset computed by the caller changes the scalar register allocation of the split-precision kernels.
template <typename R, typename I>
__device__ __forceinline__ void epi_add_res(float (&v)[4], const void* res, I row, int ld, int col, bool ok = true) {
  if (res && ok) {
    float t[4];
    load4(reinterpret_cast<const R*>(res) + (long)row * ld + col, t);
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] += t[r];
  }
}

// ---- the two-row form of the 192 x 192 (csrc/gemm_split3.hip) and 160 x 256 (csrc/gemm_f16x2_t160.hip) tiles ----
// Row-pair exchange: a, b are the accumulator fragments fn, fn + 1 of one row fragment.  Lanes fr < 8 (`lo`) trade their fn + 1 fragment for the fn
// fragment of lane fr + 8 (DPP row_ror:8, four moves); afterwards v[0], v[1] are rows fr & 7 and (fr & 7) + 8 of ONE 4-channel group (fragment fn for
// `lo` lanes, fn + 1 for the others), and every 16-byte store of a lane pair completes 128-byte lines.
__device__ __forceinline__ void epi_exchange_rows(const f32x4& a, const f32x4& b, bool lo, float (&v)[2][4]) {
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const float snd = lo ? b[r] : a[r];
    const float recv = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, snd), 0x128, 0xf, 0xf, false));   // row_ror:8
    v[0][r] = lo ? a[r] : recv;
    v[1][r] = lo ? recv : b[r];
  }
}
// fp16x2 operands: both rows * 2^e, e the four channels' exponents (col_exp).  (By value: through a reference the registers of e are zeroed in another order.)
__device__ __forceinline__ void epi_ldexp_rows(float (&v)[2][4], int4 e) {
  const int fe[4] = {e.x, e.y, e.z, e.w};
#pragma unroll
  for (int r = 0; r < 4; ++r) { v[0][r] = ldexpf(v[0][r], fe[r]); v[1][r] = ldexpf(v[1][r], fe[r]); }
}
