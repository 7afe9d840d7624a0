// fp16x2 linear layer on 160 x 256 tiles: the sibling of gemm_split3_persist192_kernel<BARE = false, BL, F16, NSL = 3> (csrc/gemm_split3.hip) for
// the ViT linears with 1024 output columns.  The kernel's body -- tile walk, piece map, three-slot ring, hand-counted waits, epilogue -- lives in
// csrc/gemm_f16x2_t160.h (persist160_body<POINTS = false>), which the points kernel of csrc/wino_f16x2_t160.hip shares; its header comment is the
// description of both.  This file holds the linear kernel and its launch.
#include "gemm_f16x2_t160.h"

namespace {

// mt / nt = token / channel tiles, total = mt * nt; tile order: token tile > channel tile (channel tile fastest)
__global__ __launch_bounds__(512) void gemm_f16x2_persist160_kernel(const pf_conv_params p, int mt, int nt, int total) {
  constexpr int NS = pf_t160::T160_SLOTS, STAGE = pf_t160::T160_STAGE;
  static_assert(NS * STAGE <= 159744, "three ring slots are the only LDS");       // (stated here too: tests/test_f16x2_tile160_resources.py reads this file)
  pf_t160::persist160_body<false>(p, mt, nt, total);
}

}  // namespace

// launch of the 160 x 256 form for a call that pf_gemm_f16x2 has validated and routed here (float32 output, no plane output).  Fewer than 8 tiles:
// 8 blocks anyway (every XCD needs a block for the walk; the blocks of an empty tile range return at once).
int pf_launch_f16x2_tile160(const pf_conv_params& p, int cus, hipStream_t st) {
  constexpr int smem = 3 * 2 * (160 + 256) * 64;
  static std::atomic<unsigned long long> done{0};
  if (!p.out_f32 || (p.korder & 48) || p.batch > 1) return PF_ERR_ARG;
  const long M = (long)p.B * p.OH * p.OW;
  const int mt = (int)((M + 159) / 160), nt = (p.Cout + 255) / 256;
  const long total = (long)mt * nt;
  const int grid = pf_launch::persist_grid(cus, 0, total, PF_GRID_ENV | PF_GRID_FLOOR8);
  if (grid < 0) return PF_ERR_ARG;
  if (!pf_ensure_dynamic_lds(done, smem, gemm_f16x2_persist160_kernel)) return PF_ERR_LAUNCH;
  hipLaunchKernelGGL(gemm_f16x2_persist160_kernel, dim3((unsigned)grid), dim3(512), smem, st, p, mt, nt, (int)total);
  return hipGetLastError() == hipSuccess ? PF_OK : PF_ERR_LAUNCH;
}
