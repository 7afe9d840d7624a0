// The batched transform-domain product of a three-step fp16x2 Winograd layer on 160 x 256 tiles: the points mode of the tile that
// csrc/gemm_f16x2_t160.hip runs for the ViT linears (shared body: csrc/gemm_f16x2_t160.h, persist160_body<POINTS = true>, whose header comment
// describes walk, ring and waits).  Same operands and the same result bits as pf_gemm_f16x2_points (192 x 192) and pf_gemm_f16x2_points128.
//
// Why this tile for these layers: N = 768 is exactly three column tiles and N = 256 one, so no padded columns are multiplied, and a V slab is read
// by 3 (1) column tiles where the 192-tile (128-tile) walk reads it 4 (2) times; a wave does 60 MFMAs per chunk for 18 fragment reads.  A Winograd
// window is 16-30 rounds of tiles, so the coarser tile does not cost a visible tail.  pf_wino_f16x2_tile (below) says which layers take it: today
// the 256-column layers with K >= 512; the 768-column layers gain per launch but not measurably in the image pass and stay on the 192-tile.
//
// This file also holds the C entry points of the mode (the launch for tests and tools, the tile decision as a query); csrc/winograd.hip run_f16x2
// calls the C++ functions.
#include "gemm_f16x2_t160.h"

namespace {

// mt / nt = token / channel tiles per point, total = batch * mt * nt; tile order: point > token tile > channel tile
__global__ __launch_bounds__(512) void gemm_f16x2_points160_kernel(const pf_conv_params p, int mt, int nt, int total) {
  pf_t160::persist160_body<true>(p, mt, nt, total);
}

}  // namespace

// launch of a call that the caller has held to f16x2_points_envelope; p.scale = the int32 column exponents [batch][w_rows].  Fewer than 8 tiles: 8
// blocks anyway (the blocks of an empty tile range return at once).
int pf_launch_f16x2_points160(const pf_conv_params& p, int cus, int grid_cap, hipStream_t st) {
  constexpr int smem = pf_t160::T160_SLOTS * pf_t160::T160_STAGE;
  static std::atomic<unsigned long long> done{0};
  const long M = (long)p.B * p.OH * p.OW;
  const int mt = (int)((M + 159) / 160), nt = (p.Cout + 255) / 256;
  const long total = (long)mt * nt * (p.batch > 1 ? p.batch : 1);
  const int grid = pf_launch::persist_grid(cus, grid_cap, total, PF_GRID_CAP | PF_GRID_FLOOR8);
  if (grid < 0) return PF_ERR_ARG;
  if (!pf_ensure_dynamic_lds(done, smem, gemm_f16x2_points160_kernel)) return PF_ERR_LAUNCH;
  hipLaunchKernelGGL(gemm_f16x2_points160_kernel, dim3((unsigned)grid), dim3(512), smem, st, p, mt, nt, (int)total);
  return hipGetLastError() == hipSuccess ? PF_OK : PF_ERR_LAUNCH;
}

// the product of one window on this tile (csrc/winograd.hip run_f16x2; pf_gemm_f16x2_points160 for tests and tools)
int pf_f16x2_points160(const pf_conv_params* p, const int* col_exp, int grid_cap, hipStream_t st) {
  if (const int rc = f16x2_points_envelope("pf_gemm_f16x2_points160", p, col_exp)) return rc;
  pf_conv_params q = *p;
  q.scale = reinterpret_cast<const float*>(col_exp);     // (int32 exponents; the kernel's epilogue reads them as such)
  const int rc = pf_launch_f16x2_points160(q, pf_cu_count(), grid_cap, st);
  return rc == PF_ERR_ARG ? pf_refuse("pf_gemm_f16x2_points160", "argument outside the envelope (include/pf_hip.h)") : rc;
}

// Does the fp16x2 product of a three-step Winograd layer run on the 160 x 256 tile (1) or on the form f16x2_points_route names (0)?  q = the product
// of the WHOLE layer (csrc/winograd.hip f16x2_layer_route), so every window size of a layer runs the same kernel; all forms give the same bits.
// PF_WINO_F16_TILE (A/B and tests, read per call): 0 = the old forms everywhere, 1 = this tile wherever the product is legal (everywhere),
// 2 = the 768-column class alone, 3 = the 256-column class alone (one class at a time for the image-pass A/B).
// THE RULE (no switch set), from profiles/r14_wino_t160_ab.md (per launch, interleaved, three rounds) and profiles/r14_wino_t160_image_ab.md:
//   Cout == 256 and Cin >= 512 (768 -> 256, 512 -> 256): MOVES.  1.21-1.29x per launch against the 128-tile kernel, won every round at every
//     window size of the pass; image pass -2.05 ms on one engine (5.0 x the largest within-arm spread, depth difference exactly 0).
//   Cout == 768 and Cin >= 512 (768 -> 768): STAYS on the 192-tile.  1.08-1.11x per launch at 2128 rows and more (1.01x and one round lost at 560
//     rows), but -0.25 ms in the image pass = 0.6 x the spread: under the bar of three times the spread, so not routed.  Switch 2 still runs it.
//   Everything else (N = 544: three column tiles for 2.1 tiles of columns; K = 256: bound by V + M bytes) was out of scope and stays.
int pf_wino_f16x2_tile(const pf_conv_params& q, int /*cus: the classes are whole column tiles, no CU count enters the rule today*/) {
  const char* s = getenv("PF_WINO_F16_TILE");
  const char mode = s ? s[0] : 'r';
  if (mode == '0') return 0;
  if (mode == '1') return 1;
  const bool wide = q.Cout == 768 && q.Cin >= 512, narrow = q.Cout == 256 && q.Cin >= 512;
  if (mode == '2') return wide;
  if (mode == '3') return narrow;
  return narrow;
}

extern "C" int pf_gemm_f16x2_points160(const pf_conv_params* p, const int* col_exp, int grid_cap, void* stream) {
  return pf_f16x2_points160(p, col_exp, grid_cap, reinterpret_cast<hipStream_t>(stream));
}

extern "C" int pf_wino_f16x2_tile_route(const pf_conv_params* p, int cus) {
  if (!p || cus <= 0) return -1;
  return pf_wino_f16x2_tile(*p, cus);
}
