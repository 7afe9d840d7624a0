// The body of the 160 x 256 fp16x2 tile, shared by its two kernels: gemm_f16x2_persist160_kernel (csrc/gemm_f16x2_t160.hip, POINTS = false: the ViT
// linears, described below) and gemm_f16x2_points160_kernel (csrc/wino_f16x2_t160.hip, POINTS = true: the batched transform-domain product of a
// three-step Winograd layer, see the end of this header comment).  Everything POINTS adds sits behind `if constexpr`: the linear kernel compiles to
// the code it was before the body moved here.
//
// fp16x2 linear layer on 160 x 256 tiles: the sibling of gemm_split3_persist192_kernel<BARE = false, BL, F16, NSL = 3> (csrc/gemm_split3.hip) for
// the ViT linears with 1024 output columns.  Operands, arithmetic and epilogue are those of the 192-tile form: x / 2^e_k and W 2^(e_k - f_n) as two
// chunk-major fp16 planes each, three products per accumulator (w_h.x_l, w_l.x_h, w_h.x_h, smallest first) on v_mfma_f32_16x16x32_f16 over the K
// chunks in ascending order, y = ldexp(acc, f_n) -> bias -> act -> LayerScale -> residual(s), float32 out.  Every output element sees the same
// products in the same order whichever tile computes it: the two forms give the same bits (tests/test_gemm_f16x2_tile160_gpu.py).
//
// Why another tile: at M = 8 x 1037 = 8296 rows and N = 1024 the 192-tile grid is 44 x 6 = 264 tiles on 256 CUs, the sixth column tile 64 columns
// wide -- every XCD has 33 tiles for 32 CUs and the launch lasts two tile times for 242 tile-units of work.  160 x 256 gives 52 x 4 = 208 full
// tiles: one round.  Eight waves as 2 (token rows) x 4 (channel columns), wave tile 80 x 64: FM = 5, FN = 4, 80 accumulator registers, 60 MFMAs
// per chunk and wave for 2 x (5 + 4) = 18 fragment reads (192-tile: 54 for 18).  pf_gemm_f16x2_route (csrc/gemm_split3.hip) picks the form.
//
// Stage = [X h 160 rows | X l 160 | W h 256 | W l 256] x 64 B = 53 248 B = 52 LDS-DMA pieces of 16 rows; three ring slots = 159 744 B, the only LDS.
// Piece q of a stage sits at byte q * 1024 of its slot (q < 20: X, else W piece q - 20).  The pieces do not split evenly into "waves 0-3 the X
// planes, waves 4-7 the W planes"; the map keeps every wave's count a compile-time constant of its group:
//   group A (waves 0-3)  PA = 6:  X pieces 5a .. 5a+4 and W piece 28 + a  (q = 48 + a)
//   group B (waves 4-7)  PB = 7:  W pieces 7b .. 7b+6                     (q = 20 + 7b + i), b = wave - 4
// Walk, ring and phases are the 192-tile kernel's BL schedule on three slots (see its header): group A runs M_A(g) in phase 2g and C_A(g) in 2g+1,
// group B M_B(g) in 2g+1 and C_B(g) in 2g+2; every wave issues its pieces of chunk g+2 at the head of its own load phase M(g) into slot (g+2) % 3,
// which held chunk g-1 (read by A in phase 2g-2, by B in 2g-1, each with lgkmcnt(0) before the phase's closing barrier), and waits for its pieces of
// chunk g+1 before the closing barrier of phase 2g+1 -- A after its MFMAs, B at the end of its load phase; A reads chunk g+1 in phase 2g+2, B in 2g+3.
// Hand-counted waits, over LDS-DMA pieces only: vmcnt(6) in group A and vmcnt(7) in group B = this wave's pieces of the newest chunk may still
// fly, everything older has landed; vmcnt(0) at the fill of a one-chunk stream and at the stream's end.  The epilogue's loads and stores are issued
// at the head of a load phase, BEFORE that phase's pieces: they are older than the pieces a counted wait lets fly, so however they retire relative
// to DMA pieces they cannot make a count pass early (never count register loads in a hand-counted wait).
// (tests/test_f16x2_tile160_model_cpu.py replays the walk, the piece map and this control flow.)
//
// POINTS: the product of pf_gemm_f16x2_points / pf_gemm_f16x2_points128 on this tile.  x = V planes [2][batch][Cin/32][M][32], w = U' planes
// [2][batch][Cin/32][w_rows][32], p.scale = int32 column exponents [batch][w_rows], y = float32 [batch][M][y_ld] = ldexp(acc, f[z][n]) and nothing
// else.  The point joins the tile index: l = (z * mt + token tile) * nt + column tile, so the nt column tiles that read one V slab are neighbours
// inside one XCD's contiguous range.  At a tile switch the loader recomputes BOTH operand bases (z moves x and w).  Same products, same term order,
// same ascending K chunks as the 192- and 128-tile forms: the same bits (tests/test_wino_f16x2_t160_gpu.py).  The exponent loads are the epilogue's
// only loads and are issued where the linear form issues its own: at the head of a load phase, before that phase's pieces.
// (tests/test_wino_f16x2_t160_model_cpu.py replays the points walk and the piece addresses.)
#pragma once
#include <atomic>
#include <cstdlib>
#include <type_traits>
#include "pf_common.h"
#include "pf_epilogue.h"
#include "../../include/pf_hip.h"
#include "pf_args.h"
#include "pf_launch.h"

namespace pf_t160 {

constexpr int T160_BM = 160, T160_BN = 256, T160_SLOTS = 3;
constexpr int T160_STAGE = 2 * (T160_BM + T160_BN) * 64;  // [X h | X l | W h | W l] rows of 64 bytes

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

// mt / nt = token / channel tiles, total = mt * nt (POINTS: x batch); tile order: (point >) token tile > channel tile (channel tile fastest)
template <bool POINTS>
__device__ __forceinline__ void persist160_body(const pf_conv_params& p, int mt, int nt, int total) {
  constexpr int BM = T160_BM, BN = T160_BN, WM = 2, WN = 4, NP = 2, NS = T160_SLOTS;
  constexpr int NW = WM * WN;
  constexpr int WTM = BM / WM, WTN = BN / WN, FM = WTM / 16, FN = WTN / 16;
  constexpr int XP = NP * BM / 16, WP = NP * BN / 16;       // 20 X pieces, 32 W pieces per stage
  constexpr int PA = 6, PB = 7, PMAX = 7;
  constexpr int STAGE = (XP + WP) * 1024;
  static_assert(4 * (PA - 1) == XP && 4 * (PB + 1) == WP && WTM % 16 == 0 && FN % 2 == 0 && NS * STAGE <= 159744 && STAGE == T160_STAGE, "piece map / ring");
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WN, wn = wave % WN;
  const int M = p.B * p.OH * p.OW;
  const int nk = p.Cin / 32;

  // ---- this block's tiles: XCD x owns the contiguous range [total x / 8, total (x+1) / 8) (the walk of the 192-tile kernel)
  const int G = (int)gridDim.x, xcd = (int)blockIdx.x & 7, nb = (G - xcd + 7) >> 3;
  const int lo = (int)((long)total * xcd / 8), hi = (int)((long)total * (xcd + 1) / 8);
  const int l_first = lo + ((int)blockIdx.x >> 3);
  if (l_first >= hi) return;
  const int my_tiles = (hi - l_first + nb - 1) / nb;
  const int chunks = my_tiles * nk;
  const int per_point = mt * nt;
  auto decode = [&](int l, int& z, int& m0, int& n0) __attribute__((always_inline)) {
    z = 0;
    if constexpr (POINTS) {                               // point slowest: l = (z * mt + token tile) * nt + channel tile
      z = l / per_point;
      l -= z * per_point;
    }
    const int t = l / nt;
    m0 = t * BM;
    n0 = (l - t * nt) * BN;
  };

  // ---- loader.  Piece i of this wave is stage piece q: lane L moves the 16 bytes of stage row 16 q + (L >> 2) at physical slot L & 3 = logical
  // slot ^ ((row >> 1) & 3) (plane origins are multiples of 8 rows: the swizzle of the stage row is the swizzle of the operand row).  Rows beyond
  // M / w_rows are clamped to the last valid row; their products land in accumulator rows / columns that are never stored.
  const bool grp_a = wave < NW / 2;
  auto piece_q = [&](int i) __attribute__((always_inline)) {
    return grp_a ? (i < PA - 1 ? wave * (PA - 1) + i : XP + 4 * PB + wave) : XP + (wave - NW / 2) * PB + i;
  };
  const unsigned x_adv = (unsigned)M * 64u, w_adv = (unsigned)p.w_rows * 64u;   // chunk-major operands: the next K chunk is one [rows][32] slab further
  unsigned long long sbase[PMAX];
  unsigned voff[PMAX];
  auto setup_loader = [&](int l) __attribute__((always_inline)) {
    int z, m0, n0;
    decode(l, z, m0, n0);
    int lane_o = lane;                                    // (opaque copy: the per-piece row constants are recomputed at every tile switch instead of
    asm volatile("" : "+v"(lane_o));                      //  being hoisted out of the chunk loop)
#pragma unroll
    for (int i = 0; i < PMAX; ++i) {
      if (grp_a && i >= PA) continue;
      const int q = piece_q(i);
      const bool is_x = q < XP;
      const int pc = is_x ? q : q - XP, ppl = is_x ? BM / 16 : BN / 16;       // piece within the operand's two planes; pieces per plane
      const int pl = pc / ppl, r = (pc - pl * ppl) * 16 + (lane_o >> 2);
      const int row = q * 16 + (lane_o >> 2);
      const int j = (lane_o & 3) ^ ((row >> 1) & 3);
      const int origin = is_x ? m0 : n0, last = (is_x ? M : p.w_rows) - 1 - origin;
      sbase[i] = (is_x ? (unsigned long long)p.x : (unsigned long long)p.w) + (unsigned long long)pl * ((is_x ? p.x_bstride : p.w_bstride) * 2ull) +
                 (unsigned long long)origin * 64ull;
      if constexpr (POINTS)                               // a point's operands: [Cin/32][rows][32] fp16 = rows * Cin * 2 bytes further per point
        sbase[i] += (unsigned long long)z * ((unsigned long long)(is_x ? M : p.w_rows) * (unsigned long long)(p.Cin * 2));
      voff[i] = (unsigned)(min(r, last) * 64 + j * 16);
    }
  };
  const unsigned smem_base = lds_addr(smem);
  int l_load = l_first, l_kc = -1, s_issue = NS - 1;
  setup_loader(l_load);
  // a whole chunk from the head of a load phase; GA: the wave's group, known at compile time in each of the two loops below
  auto issue = [&](auto ga) __attribute__((always_inline)) {
    constexpr bool GA = decltype(ga)::value;
    s_issue = s_issue + 1 == NS ? 0 : s_issue + 1;
    if (++l_kc == nk) {                                   // the stream moves on to this block's next tile
      l_kc = 0;
      l_load += nb;
      if (l_load < hi) setup_loader(l_load);
    }
    const unsigned slot_b = __builtin_amdgcn_readfirstlane(smem_base + s_issue * STAGE);
#pragma unroll
    for (int i = 0; i < (GA ? PA : PB); ++i) {
      const int q = GA ? (i < PA - 1 ? wave * (PA - 1) + i : XP + 4 * PB + wave) : XP + (wave - NW / 2) * PB + i;
      glds16s(voff[i], sbase[i], slot_b + q * 1024);
      sbase[i] += (GA && i < PA - 1) ? x_adv : w_adv;
    }
  };

  f32x4 acc[FN][FM];
#pragma unroll
  for (int fn = 0; fn < FN; ++fn)
#pragma unroll
    for (int fm = 0; fm < FM; ++fm) acc[fn][fm] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int fr = lane & 15, fg = lane >> 4;
  const int slot = (fg ^ ((fr >> 1) & 3)) << 4;          // fragment rows are multiples of 16 apart: the swizzle term is per lane
  const int x_off = (wm * WTM + fr) * 64 + slot;         // + plane * BM * 64 + fm * 1024
  const int w_off = NP * BM * 64 + (wn * WTN + fr) * 64 + slot;   // + plane * BN * 64 + fn * 1024
  struct Frags { uint4 w[NP][FN], x[NP][FM]; };
  Frags f;
  int s_read = 0;
  auto read_frags = [&]() __attribute__((always_inline)) {
    const char* S = smem + s_read * STAGE;
    s_read = s_read + 1 == NS ? 0 : s_read + 1;
#pragma unroll
    for (int pl = 0; pl < NP; ++pl) {
#pragma unroll
      for (int fn = 0; fn < FN; ++fn) f.w[pl][fn] = *reinterpret_cast<const uint4*>(S + w_off + pl * (BN * 64) + fn * 1024);
#pragma unroll
      for (int fm = 0; fm < FM; ++fm) f.x[pl][fm] = *reinterpret_cast<const uint4*>(S + x_off + pl * (BM * 64) + fm * 1024);
    }
  };
  // three partial products, smallest first (the order of the 192-tile kernel: same bits); within a term the FN * FM accumulators are independent
#define T160_TERM(PW, PX)                                                                                                     \
  _Pragma("unroll") for (int fn = 0; fn < FN; ++fn) _Pragma("unroll") for (int fm = 0; fm < FM; ++fm)                       \
      acc[fn][fm] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, f.w[PW][fn]), __builtin_bit_cast(f16x8, f.x[PX][fm]), \
                                                           acc[fn][fm], 0, 0, 0);
  auto multiply = [&]() __attribute__((always_inline)) { T160_TERM(0, 1) T160_TERM(1, 0) T160_TERM(0, 0) };
#undef T160_TERM

  int l_comp = l_first, c_kc = 0;
  int e_z = 0, e_m0 = 0, e_n0 = 0;
  bool epi_pending = false;
  // Epilogue on exchanged fragments, as in the 192-tile kernel: lanes fr < 8 trade their fn+1 fragment for the fn fragment of lane fr + 8 (DPP
  // row_ror:8); each lane then owns rows fr & 7 and (fr & 7) + 8 of ONE 4-channel group, and every 16-byte store of a lane pair completes
  // 128-byte lines.  Everything after the accumulation is elementwise, so the exchanged values take the same operations in the same order.
  auto epilogue = [&]() __attribute__((always_inline)) {
    int fr = lane & 15, fg = lane >> 4;                  // (re-derived behind an opaque barrier: everything computed from them stays INSIDE the
    asm volatile("" : "+v"(fr), "+v"(fg));               //  epilogue instead of living across the chunk loop)
    const bool lo = fr < 8;
#pragma unroll
    for (int fn = 0; fn < FN; fn += 2) {
      __builtin_amdgcn_sched_barrier(0);                 // one fragment pair at a time (register pressure)
      const int fsel = fn + (lo ? 0 : 1);                // the fragment whose values this lane stores
      const int n = e_n0 + wn * WTN + fsel * 16 + fg * 4;
      const bool nok = n < p.Cout;
      float4 bias_r = make_float4(0.f, 0.f, 0.f, 0.f), scale_r = make_float4(1.f, 1.f, 1.f, 1.f);
      int4 fexp = make_int4(0, 0, 0, 0);
      if constexpr (POINTS) {
        if (nok) fexp = *reinterpret_cast<const int4*>(reinterpret_cast<const int*>(p.scale) + (long)e_z * p.w_rows + n);
      } else if (nok) {
        fexp = *reinterpret_cast<const int4*>(p.col_exp + n);
        if (p.bias) bias_r = *reinterpret_cast<const float4*>(p.bias + n);
        if (p.scale) scale_r = *reinterpret_cast<const float4*>(p.scale + n);
      }
      const float bs[4] = {bias_r.x, bias_r.y, bias_r.z, bias_r.w}, sc[4] = {scale_r.x, scale_r.y, scale_r.z, scale_r.w};
#pragma unroll
      for (int fm = 0; fm < FM; ++fm) {
        const f32x4 a = acc[fn][fm], b = acc[fn + 1][fm];
        acc[fn][fm] = f32x4{0.f, 0.f, 0.f, 0.f};
        acc[fn + 1][fm] = f32x4{0.f, 0.f, 0.f, 0.f};
        float v[2][4];
        epi_exchange_rows(a, b, lo, v);
        const int m1 = e_m0 + wm * WTM + fm * 16 + (fr & 7);
        epi_ldexp_rows(v, fexp);
        if constexpr (POINTS) {                           // the bare store of the transform-domain product
          float* yb = reinterpret_cast<float*>(p.y) + (long)e_z * M * p.y_ld;
          if (nok && m1 < M) *reinterpret_cast<float4*>(yb + (long)m1 * p.y_ld + n) = make_float4(v[0][0], v[0][1], v[0][2], v[0][3]);
          if (nok && m1 + 8 < M) *reinterpret_cast<float4*>(yb + (long)(m1 + 8) * p.y_ld + n) = make_float4(v[1][0], v[1][1], v[1][2], v[1][3]);
          continue;
        }
#pragma unroll
        for (int h = 0; h < 2; ++h) {                     // one row at a time (register pressure)
          __builtin_amdgcn_sched_barrier(0);
          const int m = m1 + 8 * h;
          const bool ok = nok && m < M;
#pragma unroll
          for (int r = 0; r < 4; ++r) v[h][r] += bs[r];
          epi_act(v[h], p.act);
#pragma unroll
          for (int r = 0; r < 4; ++r) v[h][r] *= sc[r];
          // (written out, not epi_add_res: through the helper this kernel zeroes the residual registers in another order)
          if (p.res && ok) {
            const float4 q = *reinterpret_cast<const float4*>(reinterpret_cast<const float*>(p.res) + (long)m * p.res_ld + n);
            v[h][0] += q.x; v[h][1] += q.y; v[h][2] += q.z; v[h][3] += q.w;
          }
          if (p.res2 && ok) {
            const float4 q = *reinterpret_cast<const float4*>(reinterpret_cast<const float*>(p.res2) + (long)m * p.res2_ld + n);
            v[h][0] += q.x; v[h][1] += q.y; v[h][2] += q.z; v[h][3] += q.w;
          }
          if (ok) *reinterpret_cast<float4*>(reinterpret_cast<float*>(p.y) + (long)m * p.y_ld + n) = make_float4(v[h][0], v[h][1], v[h][2], v[h][3]);
        }
      }
    }
    epi_pending = false;
  };
  auto tile_cursor = [&]() __attribute__((always_inline)) {     // head of a load phase: stores of the finished tile, coordinates of the ending one
    if (epi_pending) epilogue();                        // beside the partner group's MFMAs
    if (c_kc == nk - 1) {
      decode(l_comp, e_z, e_m0, e_n0);
      l_comp += nb;
    }
  };
  auto tile_advance = [&]() __attribute__((always_inline)) {
    if (++c_kc == nk) { c_kc = 0; epi_pending = true; }
  };

  // ---- the chunk stream
  if (grp_a) {
    // group A: M_A(g) in phase 2g, C_A(g) in phase 2g+1
    constexpr std::true_type ga{};
    issue(ga);                                          // chunk 0
    if (chunks > 1) {
      issue(ga);                                        // chunk 1
      vm_wait<PA>();                                    // chunk 0 has landed; chunk 1 is waited for at the end of phase 1
    } else {
      vm_wait<0>();
    }
    lds_barrier();
#pragma nounroll
    for (int g = 0; g < chunks; ++g) {
      tile_cursor();
      if (g + 2 < chunks) issue(ga);                    // chunk g+2 -> slot (g+2) % 3, phase 2g
      read_frags();                                     // chunk g
      lds_barrier();
      __builtin_amdgcn_sched_barrier(0);
      __builtin_amdgcn_s_setprio(1);
      multiply();
      __builtin_amdgcn_s_setprio(0);
      tile_advance();
      if (g + 2 < chunks) vm_wait<PA>();                // this wave's pieces of chunk g+1 have landed (phase 2g+1); chunk g+2's six may fly
      else vm_wait<0>();
      plain_barrier();
    }
    plain_barrier();                                    // group B's last compute phase
  } else {
    // group B: M_B(g) in phase 2g+1 issues chunk g+2 and reads chunk g; C_B(g) in phase 2g+2 is MFMA-only
    constexpr std::false_type gb{};
    issue(gb);
    if (chunks > 1) {
      issue(gb);
      vm_wait<PB>();
    } else {
      vm_wait<0>();
    }
    lds_barrier();
    plain_barrier();                                    // phase 0 (group A's first load phase)
#pragma nounroll
    for (int g = 0; g < chunks; ++g) {
      tile_cursor();
      if (g + 2 < chunks) issue(gb);                    // chunk g+2 -> slot (g+2) % 3, phase 2g+1
      read_frags();                                     // chunk g
      if (g + 2 < chunks) vm_wait<PB>();                // chunk g+1's pieces have landed before group A reads them in phase 2g+2; chunk g+2's seven may fly
      else vm_wait<0>();
      lds_barrier();
      __builtin_amdgcn_sched_barrier(0);
      __builtin_amdgcn_s_setprio(1);
      multiply();
      __builtin_amdgcn_s_setprio(0);
      tile_advance();
      plain_barrier();
    }
  }
  epilogue();
}

}  // namespace pf_t160
