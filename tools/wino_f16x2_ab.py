"""Interleaved A/B of the fp16x2 three-step Winograd layer against the bf16x3 one, in ONE process, HIP events, cold caches before every timed launch:
  gemm   the batched transform-domain product alone on one window of the headline layer (544->544 @ 8x392x518: 13 632 tiles, 36 points):
         gemm_split3_persist192_kernel (3 bf16 planes, six MFMAs per product) vs its fp16x2 form (2 fp16 planes, three) on random operands, the
         fp16x2 form on its three-slot ring (default) and on two slots (PF_F16_SLOTS=2)
  layer  the whole layer call through HipOps.conv, PF_WINO_F16X2=0 vs 1 (pre-pass and U' split included), and max |y1 - y0| / max |y0|
usage: python tools/wino_f16x2_ab.py [--rounds R] [--reps N] [--B 8 --H 392 --W 518 --C 544] [--gemm-only N]
       --gemm-only N: N launches of the fp16x2 product and nothing else (a command for rocprofv3 counter passes)"""
import argparse
import ctypes as C
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--B", type=int, default=8)
    ap.add_argument("--H", type=int, default=392)
    ap.add_argument("--W", type=int, default=518)
    ap.add_argument("--C", type=int, default=544)
    ap.add_argument("--gemm-only", type=int, default=0)
    a = ap.parse_args()
    from patchfusion_amd import _lib, hip_ops
    from patchfusion_amd import packing as pk
    from patchfusion_amd.hip_ops import ops
    L = _lib.load()
    dev = torch.device("cuda", 0)
    flush = torch.empty(256 * 2 ** 20, dtype=torch.float32, device=dev)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def timed(fn):
        flush.add_(1.0)
        ev[0].record()
        fn()
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1])

    B, H, W, Cc = a.B, a.H, a.W, a.C
    g = torch.Generator().manual_seed(0)
    w = torch.randn(Cc, Cc, 3, 3, generator=g) / (9 * Cc) ** 0.5
    pw = pk.pack_conv(w, torch.randn(Cc, generator=g), dtype=torch.float32).to(dev)
    window = hip_ops.wino3_window(B, H, W, pw)[0]
    rows = pw.wino_u.shape[1]

    # ---- the product alone, one window
    T = window
    q = _lib.ConvParams()
    q.x_ld, q.B, q.H, q.W, q.Cin, q.w_rows, q.Kpad = Cc, 1, 1, T, Cc, rows, Cc
    q.y_ld, q.OH, q.OW, q.Cout, q.KH, q.KW, q.stride, q.pad = Cc, 1, T, Cc, 1, 1, 1, 0
    q.act, q.shuffle, q.dtype, q.out_f32, q.korder, q.batch = 0, 1, 1, 1, 6, 36
    V3 = torch.randn(3, 36, Cc // 32, T, 32, device=dev).bfloat16()
    V2 = torch.randn(2, 36, Cc // 32, T, 32, device=dev).half()
    U2 = torch.randn(2, 36, Cc // 32, rows, 32, device=dev).half()
    fe = torch.zeros(36, rows, dtype=torch.int32, device=dev)
    M = torch.empty(36, T, Cc, device=dev)

    def g3():
        q.x, q.w, q.y = V3.data_ptr(), pw.wino_u3.data_ptr(), M.data_ptr()
        q.x_bstride, q.w_bstride = 36 * T * Cc, 36 * rows * Cc
        hip_ops.check(L.pf_gemm_split3_ex(C.byref(q), 0, None), "pf_gemm_split3_ex")

    def g2():
        q.x, q.w, q.y = V2.data_ptr(), U2.data_ptr(), M.data_ptr()
        q.x_bstride, q.w_bstride = 36 * T * Cc, 36 * rows * Cc
        hip_ops.check(L.pf_gemm_f16x2_points(C.byref(q), C.c_void_p(fe.data_ptr()), 0, None), "pf_gemm_f16x2_points")

    def g2s2():                                            # the fp16x2 kernel on the two-slot ring (PF_F16_SLOTS=2, read per call)
        os.environ["PF_F16_SLOTS"] = "2"
        g2()
        os.environ.pop("PF_F16_SLOTS")

    if a.gemm_only:
        for _ in range(a.gemm_only):
            g2()
        torch.cuda.synchronize()
        print(f"{a.gemm_only} launches of the fp16x2 product, {T} tiles x 36 points, {Cc}->{Cc}")
        return

    for f in (g3, g2, g2s2, g3, g2, g2s2):
        f()
    torch.cuda.synchronize()
    t3, t2, t22 = [], [], []
    for _ in range(a.rounds):
        for _ in range(a.reps):
            t3.append(timed(g3))
            t2.append(timed(g2))
            t22.append(timed(g2s2))
    m3, m2, m22 = statistics.median(t3), statistics.median(t2), statistics.median(t22)
    flops = 2.0 * 36 * T * Cc * Cc
    print(f"gemm {T} tiles x 36 points, {Cc}->{Cc}: bf16x3 {m3:.3f} ms ({flops / m3 / 1e9:.0f} useful TF/s)  fp16x2 {m2:.3f} ms "
          f"({flops / m2 / 1e9:.0f})  speed-up {m3 / m2:.3f}x  (medians of {len(t3)}; min {min(t3):.3f} / {min(t2):.3f}); "
          f"fp16x2 on two ring slots {m22:.3f} ms ({m3 / m22:.3f}x)")
    del V3, V2, U2, M
    torch.cuda.empty_cache()

    # ---- the whole layer call
    x = torch.randn(B, H, W, Cc, generator=g).to(dev)
    y = torch.empty(B, H, W, Cc, device=dev)

    def layer(mode):
        os.environ["PF_WINO_F16X2"] = mode
        hip_ops.refresh_env()
        ops.conv(x, pw, y, pad=1, act="relu")
        torch.cuda.synchronize()

    res = {}
    for mode in ("0", "1"):
        layer(mode)
        res[mode] = y.clone()
    err = float((res["1"] - res["0"]).abs().max() / res["0"].abs().max())
    del res
    tl = {"0": [], "1": []}
    for _ in range(a.rounds):
        for mode in ("0", "1"):
            os.environ["PF_WINO_F16X2"] = mode
            hip_ops.refresh_env()
            ops.conv(x, pw, y, pad=1, act="relu")          # (plan + arena growth outside the timed call)
            for _ in range(a.reps):
                tl[mode].append(timed(lambda: ops.conv(x, pw, y, pad=1, act="relu")))
    l0, l1 = statistics.median(tl["0"]), statistics.median(tl["1"])
    print(f"layer {Cc}->{Cc} @ {B}x{H}x{W} (window {window} tiles): bf16x3 {l0:.2f} ms  fp16x2 {l1:.2f} ms  speed-up {l0 / l1:.3f}x  "
          f"(medians of {len(tl['0'])}); max |y16 - y3| / max |y3| = {err:.2e}")


if __name__ == "__main__":
    main()
