"""Interleaved A/B of the batched fp16x2 transform-domain product of the three-step Winograd layers: the form the layer runs today (192 x 192 tiles,
pf_gemm_f16x2_points, for N = 768; 128 x 128 tiles, pf_gemm_f16x2_points128, for N = 256) against the 160 x 256 tile (pf_gemm_f16x2_points160,
csrc/wino_f16x2_t160.hip).  The protocol of tools/wino_n256_ab.py: ONE process, HIP events, cold caches before every timed launch, an untimed round
first, then R timed rounds with the arms interleaved launch by launch; EVERY round is shown (its median over the reps), and "won every round" is a
column.  Shapes = (K, N, rows of one window) as the 4K image pass issues them.  Random planes, random column exponents; the two arms must give the
same bits, which is checked before anything is timed.
usage: python tools/wino_t160_ab.py [--rounds R] [--reps N] [--only K,N,T] [--launches N --arm old|new]
       (--launches: N launches of one arm on the --only shape and nothing else: a command for rocprofv3 counter passes)"""
import argparse
import ctypes as C
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [(768, 768, 9600), (768, 768, 8288), (768, 768, 2128), (768, 768, 560), (768, 256, 13056), (768, 256, 8288), (512, 256, 18048), (512, 256, 8288)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default="")
    ap.add_argument("--launches", type=int, default=0)
    ap.add_argument("--arm", default="new")
    a = ap.parse_args()
    from patchfusion_amd import _lib, hip_ops
    L = _lib.load()
    dev = torch.device("cuda", 0)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    shapes = [tuple(int(v) for v in a.only.split(","))] if a.only else SHAPES

    def product(K, N, T):
        g = torch.Generator(device=dev).manual_seed(K + N + T)
        q = _lib.ConvParams()
        q.x_ld, q.B, q.H, q.W, q.Cin, q.w_rows, q.Kpad = K, 1, 1, T, K, N, K
        q.y_ld, q.OH, q.OW, q.Cout, q.KH, q.KW, q.stride, q.pad = N, 1, T, N, 1, 1, 1, 0
        q.act, q.shuffle, q.dtype, q.out_f32, q.korder, q.batch = 0, 1, 1, 1, 6, 36
        V2 = torch.randn(2, 36, K // 32, T, 32, device=dev, generator=g).half()
        U2 = torch.randn(2, 36, K // 32, N, 32, device=dev, generator=g).half()
        fe = torch.randint(-12, 13, (36, N), dtype=torch.int32, device=dev, generator=g)
        M = torch.empty(36, T, N, device=dev)
        q.x, q.w, q.y, q.x_bstride, q.w_bstride = V2.data_ptr(), U2.data_ptr(), M.data_ptr(), 36 * T * K, 36 * N * K
        old_fn, old_nm = (L.pf_gemm_f16x2_points128, "pf_gemm_f16x2_points128") if N <= 256 else (L.pf_gemm_f16x2_points, "pf_gemm_f16x2_points")

        def old():
            hip_ops.check(old_fn(C.byref(q), C.c_void_p(fe.data_ptr()), 0, None), old_nm)

        def new():
            hip_ops.check(L.pf_gemm_f16x2_points160(C.byref(q), C.c_void_p(fe.data_ptr()), 0, None), "pf_gemm_f16x2_points160")
        return old, new, M, (V2, U2, fe, q)

    if a.launches:
        K, N, T = shapes[0]
        old, new, M, keep = product(K, N, T)
        for _ in range(a.launches):
            (old if a.arm == "old" else new)()
        torch.cuda.synchronize()
        print(f"{a.launches} launches of the {a.arm} arm, {K}->{N} @ {T} rows")
        return

    flush = torch.empty(256 * 2 ** 20, dtype=torch.float32, device=dev)

    def timed(fn):
        flush.add_(1.0)
        ev[0].record()
        fn()
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1])

    rounds_hdr = " | ".join(f"round {r + 1} old / new ms" for r in range(a.rounds))
    print(f"| product | rows | old form | {rounds_hdr} | median old ms | median new ms | x | won every round | same bits |")
    print("|---|---:|---|" + "---:|" * a.rounds + "---:|---:|---:|---|---|")
    for K, N, T in shapes:
        old, new, M, keep = product(K, N, T)
        M.fill_(float("nan"))
        old()
        torch.cuda.synchronize()
        want = M.clone()
        M.fill_(float("nan"))
        new()
        torch.cuda.synchronize()
        same = bool(torch.equal(want.view(torch.int32), M.view(torch.int32)))
        del want
        for f in (old, new, old, new):                       # the untimed round
            timed(f)
        per_round, t_old, t_new = [], [], []
        for _ in range(a.rounds):
            ro, rn = [], []
            for _ in range(a.reps):
                ro.append(timed(old))
                rn.append(timed(new))
            per_round.append((statistics.median(ro), statistics.median(rn)))
            t_old += ro
            t_new += rn
        mo, mn = statistics.median(t_old), statistics.median(t_new)
        won = all(n < o for o, n in per_round)
        cells = " | ".join(f"{o:.3f} / {n:.3f}" for o, n in per_round)
        print(f"| {K}->{N} | {T} | {'128' if N <= 256 else '192'}-tile | {cells} | {mo:.3f} | {mn:.3f} | {mo / mn:.2f} | {'yes' if won else 'no'} | {'yes' if same else 'NO'} |",
              flush=True)
        del old, new, M, keep
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
