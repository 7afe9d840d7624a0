"""Interleaved A/B of the 256-column three-step Winograd layers: the 128-tile bf16x3 product (gemm_split3_persist_kernel) against its fp16x2 form
(csrc/wino_f16x2_n256.hip), in ONE process, HIP events, cold caches before every timed launch, an untimed pass first (profiles/r5_sweep_order_bias.md).
Per shape: `gemm` = the batched transform-domain product alone on one window, random planes; `layer` = the whole call through HipOps.conv with
PF_WINO_F16X2_N256=0 / 3 (3 = every 128-tile layer, whatever the default rule says; range pass and U' split included), the fp16x2 layer again with
the channel maxima GIVEN (what a producer's output transform hands over: no memset, no range pass; the difference is the range pass), and
max |y1 - y0| / max |y0|.  The bf16x3 product goes through pf_gemm_split3_ex and so through its own route: 1024->256 @ 8x28x37 runs the ONE-TILE
128 x 128 kernel there, not the persistent walk.  Prints one markdown table row per shape.
usage: python tools/wino_n256_ab.py [--rounds R] [--reps N] [--gemm-only N] [--old]   (--gemm-only: N launches of one product on 512->256 @ 8x56x74 and
       nothing else, --old = the bf16x3 kernel: a command for rocprofv3 counter passes)"""
import argparse
import ctypes as C
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [(768, 224, 296), (512, 224, 296), (256, 224, 296), (256, 196, 259), (768, 112, 148), (512, 112, 148), (256, 112, 148), (256, 98, 129),
          (512, 56, 74), (1024, 28, 37)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--gemm-only", type=int, default=0)
    ap.add_argument("--old", action="store_true")
    a = ap.parse_args()
    from patchfusion_amd import _lib, hip_ops
    from patchfusion_amd import packing as pk
    from patchfusion_amd.hip_ops import HipOps, ops
    L = _lib.load()
    dev = torch.device("cuda", 0)
    flush = torch.empty(256 * 2 ** 20, dtype=torch.float32, device=dev)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    B, N = 8, 256

    def timed(fn):
        flush.add_(1.0)
        ev[0].record()
        fn()
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1])

    def product(K, T, rows, u3):
        q = _lib.ConvParams()
        q.x_ld, q.B, q.H, q.W, q.Cin, q.w_rows, q.Kpad = K, 1, 1, T, K, rows, K
        q.y_ld, q.OH, q.OW, q.Cout, q.KH, q.KW, q.stride, q.pad = N, 1, T, N, 1, 1, 1, 0
        q.act, q.shuffle, q.dtype, q.out_f32, q.korder, q.batch = 0, 1, 1, 1, 6, 36
        V3 = torch.randn(3, 36, K // 32, T, 32, device=dev).bfloat16()
        V2 = torch.randn(2, 36, K // 32, T, 32, device=dev).half()
        U2 = torch.randn(2, 36, K // 32, rows, 32, device=dev).half()
        fe = torch.zeros(36, rows, dtype=torch.int32, device=dev)
        M = torch.empty(36, T, N, device=dev)
        q.y, q.x_bstride, q.w_bstride = M.data_ptr(), 36 * T * K, 36 * rows * K

        def g3():
            q.x, q.w = V3.data_ptr(), u3.data_ptr()
            hip_ops.check(L.pf_gemm_split3_ex(C.byref(q), 0, None), "pf_gemm_split3_ex")

        def g2():
            q.x, q.w = V2.data_ptr(), U2.data_ptr()
            hip_ops.check(L.pf_gemm_f16x2_points128(C.byref(q), C.c_void_p(fe.data_ptr()), 0, None), "pf_gemm_f16x2_points128")
        return g3, g2, (V3, V2, U2, fe, M, q)

    if a.gemm_only:
        K, H, W = 512, 56, 74
        g = torch.Generator().manual_seed(0)
        pw = pk.pack_conv(torch.randn(N, K, 3, 3, generator=g) / (9 * K) ** 0.5, torch.randn(N, generator=g), dtype=torch.float32).to(dev)
        g3, g2, keep = product(K, hip_ops.wino3_window(B, H, W, pw)[0], pw.wino_u.shape[1], pw.wino_u3)
        for _ in range(a.gemm_only):
            (g3 if a.old else g2)()
        torch.cuda.synchronize()
        print(f"{a.gemm_only} launches of the {'bf16x3' if a.old else 'fp16x2'} 128-tile product, {K}->{N} @ {B}x{H}x{W}")
        return

    print("| layer | tiles | route | gemm bf16x3 ms | gemm fp16x2 ms | gemm x | layer bf16x3 ms | layer fp16x2 ms | layer x | layer fp16x2, maxima given ms | x | max rel diff |")
    print("|---|---:|---|---:|---:|---:|---:|---:|---:|---:|---:|---:|")
    for K, H, W in SHAPES:
        g = torch.Generator().manual_seed(K + H)
        pw = pk.pack_conv(torch.randn(N, K, 3, 3, generator=g) / (9 * K) ** 0.5, torch.randn(N, generator=g), dtype=torch.float32).to(dev)
        T = hip_ops.wino3_window(B, H, W, pw)[0]
        g3, g2, keep = product(K, T, pw.wino_u.shape[1], pw.wino_u3)
        for f in (g3, g2, g3, g2):
            f()
        torch.cuda.synchronize()
        t3, t2 = [], []
        for _ in range(a.rounds):
            for _ in range(a.reps):
                t3.append(timed(g3))
                t2.append(timed(g2))
        del g3, g2, keep
        torch.cuda.empty_cache()
        x = torch.randn(B, H, W, K, generator=g).to(dev)
        y = torch.empty(B, H, W, N, device=dev)
        res, tl, routes = {}, {"0": [], "1": []}, {}
        for mode in ("0", "1"):
            os.environ["PF_WINO_F16X2_N256"] = "3" if mode == "1" else mode
            hip_ops.refresh_env()
            routes[mode] = HipOps._conv_plan(x, pw, y, 1, 1, "relu", False, None, None, None)[0]
            ops.conv(x, pw, y, pad=1, act="relu")
            torch.cuda.synchronize()
            res[mode] = y.clone()
        err = float((res["1"] - res["0"]).abs().max() / res["0"].abs().max())
        del res
        for _ in range(a.rounds):
            for mode in ("0", "1"):
                os.environ["PF_WINO_F16X2_N256"] = "3" if mode == "1" else mode
                hip_ops.refresh_env()
                ops.conv(x, pw, y, pad=1, act="relu")          # (plan + arena growth outside the timed call)
                for _ in range(a.reps):
                    tl[mode].append(timed(lambda: ops.conv(x, pw, y, pad=1, act="relu")))
        lg = []
        if routes["1"] == "wino3h":                            # (still in mode 3) the same layer with the maxima handed in
            cm = torch.zeros(K, dtype=torch.int32, device=dev)
            hip_ops.check(L.pf_wino_absmax(C.c_void_p(x.data_ptr()), K, B * H * W, K, 0, C.c_void_p(cm.data_ptr()), None), "pf_wino_absmax")
            ent = HipOps._conv_plan(x, pw, y, 1, 1, "relu", False, None, None, None)
            run = lambda: HipOps._conv_exec(ent[0], ent[1], ent[2], dev, cmax_in=cm)
            run()
            for _ in range(a.rounds * a.reps):
                lg.append(timed(run))
        os.environ.pop("PF_WINO_F16X2_N256")
        m3, m2, l0, l1 = (statistics.median(v) for v in (t3, t2, tl["0"], tl["1"]))
        lgm = statistics.median(lg) if lg else float("nan")
        print(f"| {K}->{N} @ {B}x{H}x{W} | {T} | {routes['0']} / {routes['1']} | {m3:.3f} | {m2:.3f} | {m3 / m2:.2f} | {l0:.3f} | {l1:.3f} | {l0 / l1:.2f} | {lgm:.3f} | {l0 / lgm:.2f} | {err:.1e} |",
              flush=True)
        del x, y, pw
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
