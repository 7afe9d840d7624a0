"""GPU probe of the fp16x2 ViT block linears (pf_gemm_f16x2) against the bf16x3 ones (pf_gemm_split3).
usage: python tools/vit_f16x2_ab.py linears            each linear at the pass's token counts, both routes interleaved in one process (untimed round,
                                                        then R rounds of 20 launches per route; best round), producer LayerNorm timed alongside
       python tools/vit_f16x2_ab.py image [--steps K] [--rounds R]   whole image pass (BASELINE configs[2]), one engine per route (PF_VIT_F16X2 is read
                                                        at engine build), routes interleaved round by round; max |depth difference|
       python tools/vit_f16x2_ab.py tiles              the 160 x 256 tile form (csrc/gemm_f16x2_t160.hip, PF_F16_TILE=1) against the 192 x 192 form (=0) per launch at
                                                        8296 rows, float32 out: fc2 and proj (also on the bf16x3 128-tile route), qkv's and fc1's shapes; every round printed
       python tools/vit_f16x2_ab.py fc2                six fc2 launches (8296 rows) on each tile form and nothing else: the target of a counter run
                                                        (rocprofv3 --pmc ... -- python tools/vit_f16x2_ab.py fc2, no tracing beside it)
       python tools/vit_f16x2_ab.py tile_image [--steps K] [--rounds R] [--reverse]   whole image pass, three arms interleaved round by round: PF_F16_TILE=0 (192-tiles everywhere),
                                                        default routing (fc2 on the new tile), default routing with PF_VIT_ATTN_F16X2=2 (fc2 and an fp16x2 proj)
       python tools/vit_f16x2_ab.py slack [--wide]      per layer log2(static bound / observed max) of the K-side operands over one image pass
                                                        (min and median over channels); --wide: tests/dynamic_range.py weights"""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEV = "cuda"


def _timed(fn, iters=20):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def linears(rounds):
    from patchfusion_amd import packing as pk
    from patchfusion_amd.hip_ops import ops
    g = torch.Generator().manual_seed(0)
    D = 1024
    print("| op | M | bf16x3 ms | fp16x2 ms | speed-up |")
    print("|---|---|---|---|---|")
    for M in (8 * 1037, 1037):
        x = torch.randn(M, D, generator=g).to(DEV)
        gam, bet = torch.randn(D, generator=g), torch.randn(D, generator=g)
        bound = pk.layernorm_bound(gam, bet)
        gd, bd = gam.to(DEV), bet.to(DEV)
        h3 = torch.empty(3, D // 32, M, 32, dtype=torch.bfloat16, device=DEV)
        for name, K, N, act, res, scale in (("qkv", D, 3 * D, None, False, False), ("fc1", D, 4 * D, "gelu", False, False),
                                            ("fc2", 4 * D, D, None, True, True)):
            w = torch.randn(N, K, generator=g) / K ** 0.5
            b = torch.randn(N, generator=g)
            sc = (0.5 + torch.rand(N, generator=g)) if scale else None
            kb = bound if K == D else pk.gelu_linear_bound(torch.randn(K, D, generator=g) / D ** 0.5, torch.randn(K, generator=g), bound)
            pw3 = pk.pack_conv_split3(w, b, scale=sc, kmajor=True).to(DEV)
            pw2 = pk.pack_conv_f16x2(w, b, sc, kb).to(DEV)
            x3 = torch.randn(3, K // 32, M, 32, generator=g).to(torch.bfloat16).to(DEV)
            x2 = torch.randn(2, K // 32, M, 32, generator=g).to(torch.float16).to(DEV)
            r = torch.randn(M, N, generator=g).to(DEV) if res else None
            if name == "qkv":
                y3 = torch.empty(3, M, N, dtype=torch.bfloat16, device=DEV)
                y2, oe = y3, None
            elif name == "fc1":
                y3 = torch.empty(3, N // 32, M, 32, dtype=torch.bfloat16, device=DEV)
                y2 = torch.empty(2, N // 32, M, 32, dtype=torch.float16, device=DEV)
                oe = torch.full((N,), -6, dtype=torch.int32, device=DEV)
            else:
                y3 = y2 = torch.empty(M, N, device=DEV)
                oe = None
            arms = [lambda: ops.conv_split3(x3, pw3, y3, act=act, res=r), lambda: ops.conv_f16x2(x2, pw2, y2, act=act, res=r, out_exp=oe)]
            best = [1e9, 1e9]
            for rnd in range(rounds + 1):
                for i, f in enumerate(arms):
                    t = _timed(f)
                    if rnd:
                        best[i] = min(best[i], t)
            print(f"| {name} {K}->{N} | {M} | {best[0]:.4f} | {best[1]:.4f} | {best[0] / best[1]:.2f}x |", flush=True)
        h2 = torch.empty(2, D // 32, M, 32, dtype=torch.float16, device=DEV)
        ie = pk.bound_exponents(bound).to(DEV)
        arms = [lambda: ops.layernorm_split3(x, h3, gd, bd, 1e-6), lambda: ops.layernorm_f16x2(x, h2, gd, bd, 1e-6, ie)]
        best = [1e9, 1e9]
        for rnd in range(rounds + 1):
            for i, f in enumerate(arms):
                t = _timed(f)
                if rnd:
                    best[i] = min(best[i], t)
        print(f"| LayerNorm -> planes {D} | {M} | {best[0]:.4f} | {best[1]:.4f} | {best[0] / best[1]:.2f}x |", flush=True)


def tiles(rounds):
    from patchfusion_amd import packing as pk
    from patchfusion_amd.hip_ops import ops
    g = torch.Generator().manual_seed(0)
    D, M = 1024, 8 * 1037
    print("| op | arm | " + " | ".join(f"round {r} ms" for r in range(rounds)) + " | best ms |")
    print("|---|---|" + "---|" * (rounds + 1))
    for name, K, N, res, scale in (("fc2", 4 * D, D, True, True), ("proj", D, D, True, True), ("qkv shape, float32 out", D, 3 * D, False, False),
                                   ("fc1 shape, float32 out", D, 4 * D, False, False)):
        w = torch.randn(N, K, generator=g) / K ** 0.5
        b = torch.randn(N, generator=g)
        sc = (0.5 + torch.rand(N, generator=g)) if scale else None
        pw3 = pk.pack_conv_split3(w, b, scale=sc, kmajor=True).to(DEV)
        pw2 = pk.pack_conv_f16x2(w, b, sc, torch.full((K,), 8.0, dtype=torch.float64)).to(DEV)
        x3 = torch.randn(3, K // 32, M, 32, generator=g).to(torch.bfloat16).to(DEV)
        x2 = torch.randn(2, K // 32, M, 32, generator=g).to(torch.float16).to(DEV)
        r = torch.randn(M, N, generator=g).to(DEV) if res else None
        y = torch.empty(M, N, device=DEV)

        def f16(tile):
            def run():
                os.environ["PF_F16_TILE"] = tile
                ops.conv_f16x2(x2, pw2, y, res=r)
            return run
        arms = [("bf16x3 (pf_gemm_split3 route)", lambda: ops.conv_split3(x3, pw3, y, res=r)), ("fp16x2 192 x 192", f16("0")), ("fp16x2 160 x 256", f16("1"))]
        times = [[] for _ in arms]
        for rnd in range(rounds + 1):
            for i, (_, f) in enumerate(arms):
                t = _timed(f)
                if rnd:
                    times[i].append(t)
        for (an, _), ts in zip(arms, times):
            print(f"| {name} {K}->{N} | {an} | " + " | ".join(f"{t:.4f}" for t in ts) + f" | {min(ts):.4f} |", flush=True)
    os.environ.pop("PF_F16_TILE", None)


def fc2_only():
    from patchfusion_amd import packing as pk
    from patchfusion_amd.hip_ops import ops
    g = torch.Generator().manual_seed(0)
    D, M = 1024, 8 * 1037
    K, N = 4 * D, D
    pw2 = pk.pack_conv_f16x2(torch.randn(N, K, generator=g) / K ** 0.5, torch.randn(N, generator=g), 0.5 + torch.rand(N, generator=g),
                             torch.full((K,), 8.0, dtype=torch.float64)).to(DEV)
    x2 = torch.randn(2, K // 32, M, 32, generator=g).to(torch.float16).to(DEV)
    r = torch.randn(M, N, generator=g).to(DEV)
    y = torch.empty(M, N, device=DEV)
    for tile in ("0", "1"):
        os.environ["PF_F16_TILE"] = tile
        for _ in range(6):
            ops.conv_f16x2(x2, pw2, y, res=r)
        torch.cuda.synchronize()
    os.environ.pop("PF_F16_TILE", None)


def tile_image(steps, rounds, reverse=False):
    from patchfusion_amd.config import make_config
    from patchfusion_amd.spec import patchfusion_spec, synthetic_state_dict
    dev = torch.device("cuda", 0)
    cfg = make_config("vitl", (392, 518), (2160, 3840), (4, 4))
    sd = synthetic_state_dict(patchfusion_spec(cfg), 0)
    img = torch.rand(1, 3, 2160, 3840, generator=torch.Generator().manual_seed(1234)).to(dev)
    os.environ.pop("PF_F16_TILE", None)
    models = {}
    # PF_VIT_ATTN_F16X2 is read when the engine is built (first forward); PF_F16_TILE per call.  The engine built second has run slower whichever arm
    # it holds (profiles/r10_attn_f16x2_image_ab.md): --reverse builds the PF_VIT_ATTN_F16X2=2 engine first, and a verdict on that arm needs both orders
    for v in (("2", "1") if reverse else ("1", "2")):
        os.environ["PF_VIT_ATTN_F16X2"] = v
        m = _model(sd, cfg, dev)
        lr = m.resizer(img)
        m(mode="infer", image_lr=lr, image_hr=img, cai_mode="m1", process_num=8)
        torch.cuda.synchronize()
        models[v] = m
    os.environ.pop("PF_VIT_ATTN_F16X2", None)
    assert [models[v]._engine["fine"].proj_f16x2 for v in ("1", "2")] == [False, True]
    arms = [("PF_F16_TILE=0, PF_VIT_ATTN_F16X2=1 (the 192-tile everywhere)", "1", "0"), ("default routing, PF_VIT_ATTN_F16X2=1 (fc2 moves)", "1", None),
            ("default routing, PF_VIT_ATTN_F16X2=2 (fc2 and proj move)", "2", None)]

    def run(arm):
        _, eng, tile = arm
        if tile is None:
            os.environ.pop("PF_F16_TILE", None)
        else:
            os.environ["PF_F16_TILE"] = tile
        d, _ = models[eng](mode="infer", image_lr=lr, image_hr=img, cai_mode="m1", process_num=8)
        return d
    for arm in arms:                                     # one untimed round
        run(arm)
    torch.cuda.synchronize()
    times, outs = [[] for _ in arms], [None for _ in arms]
    for r in range(rounds):
        for i, arm in enumerate(arms):
            outs[i] = run(arm).clone()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                run(arm)
            torch.cuda.synchronize()
            times[i].append((time.perf_counter() - t0) / steps * 1e3)
            print(f"round {r} {arm[0]}: {times[i][-1]:.2f} ms", file=sys.stderr, flush=True)
    os.environ.pop("PF_F16_TILE", None)
    print("| arm | " + " | ".join(f"round {r} ms" for r in range(rounds)) + " | mean ms | spread ms | vs arm 0 | max abs depth diff vs arm 0 |")
    print("|---|" + "---|" * (rounds + 4))
    m0 = sum(times[0]) / rounds
    for i, arm in enumerate(arms):
        m = sum(times[i]) / rounds
        print(f"| {arm[0]} | " + " | ".join(f"{t:.2f}" for t in times[i]) + f" | {m:.2f} | {max(times[i]) - min(times[i]):.2f} | {m - m0:+.2f} | "
              f"{float((outs[i] - outs[0]).abs().max()):.3e} |")
    spread = max(max(t) - min(t) for t in times)
    for i in range(1, len(arms)):
        gain = m0 - sum(times[i]) / rounds
        print(f"\narm {i} against arm 0: gain {gain:.2f} ms, largest within-arm spread {spread:.2f} ms, ratio {gain / spread:.1f} (rule: >= 3)")
    print(f"\n{steps} images per cell, split 4x4, process_num 8, depth max {float(outs[0].abs().max()):.3f}; engines built in the order "
          f"PF_VIT_ATTN_F16X2={'2, 1' if reverse else '1, 2'}")


def _model(sd, cfg, dev):
    from patchfusion_amd.model import PatchFusion
    m = PatchFusion(cfg, compute_dtype="fp32").eval()
    m.load_state_dict(sd, strict=True)
    return m.to(dev)


def image(steps, rounds):
    from patchfusion_amd.config import make_config
    from patchfusion_amd.spec import patchfusion_spec, synthetic_state_dict
    dev = torch.device("cuda", 0)
    cfg = make_config("vitl", (392, 518), (2160, 3840), (4, 4))
    sd = synthetic_state_dict(patchfusion_spec(cfg), 0)
    img = torch.rand(1, 3, 2160, 3840, generator=torch.Generator().manual_seed(1234)).to(dev)
    arms, models = ("0", "1"), []
    for v in arms:                                       # the route is fixed when the engine is built (first forward)
        os.environ["PF_VIT_F16X2"] = v
        m = _model(sd, cfg, dev)
        lr = m.resizer(img)
        m(mode="infer", image_lr=lr, image_hr=img, cai_mode="m1", process_num=8)
        models.append(m)
    assert [m._engine["fine"].f16x2 for m in models] == [False, True]
    times, outs = [[], []], [None, None]
    for r in range(rounds):
        for i, m in enumerate(models):
            d, _ = m(mode="infer", image_lr=lr, image_hr=img, cai_mode="m1", process_num=8)
            torch.cuda.synchronize()
            outs[i] = d.clone()
            t0 = time.perf_counter()
            for _ in range(steps):
                m(mode="infer", image_lr=lr, image_hr=img, cai_mode="m1", process_num=8)
            torch.cuda.synchronize()
            times[i].append((time.perf_counter() - t0) / steps * 1e3)
            print(f"round {r} PF_VIT_F16X2={arms[i]}: {times[i][-1]:.2f} ms", file=sys.stderr, flush=True)
    print("| variant | " + " | ".join(f"round {r} ms" for r in range(rounds)) + " | mean ms | vs PF_VIT_F16X2=0 |")
    print("|---|" + "---|" * (rounds + 2))
    m0 = sum(times[0]) / rounds
    for i, v in enumerate(arms):
        m = sum(times[i]) / rounds
        print(f"| `PF_VIT_F16X2={v}` | " + " | ".join(f"{t:.2f}" for t in times[i]) + f" | {m:.2f} | {m - m0:+.2f} |")
    print(f"\nmax |depth(fp16x2) - depth(bf16x3)| = {float((outs[1] - outs[0]).abs().max()):.3e} (depth max {float(outs[0].abs().max()):.3f}); "
          f"{steps} images per cell, split 4x4, process_num 8")


class _Recorder:
    """the HIP op set, with the K-side operands of the fp16x2 linears read back after each call: per channel max |value| against the bound"""

    def __init__(self, ops):
        self._ops, self.rows = ops, {}

    def __getattr__(self, k):
        return getattr(self._ops, k)

    def _take(self, key, planes, exp, bound):
        v = torch.ldexp(planes.float().sum(0).permute(1, 0, 2).reshape(planes.shape[2], -1).double(), exp.double()[None, :])
        mx = v.abs().amax(0).cpu()
        self.rows.setdefault(key, []).append((mx, bound))

    def layernorm_f16x2(self, x, y2, g, b, eps, in_exp):
        self._ops.layernorm_f16x2(x, y2, g, b, eps, in_exp)
        from patchfusion_amd import packing as pk
        self._take("LN -> qkv / fc1", y2, in_exp, pk.layernorm_bound(g, b))

    def conv_f16x2(self, x2, pw, y, act=None, res=None, res2=None, out_exp=None):
        self._ops.conv_f16x2(x2, pw, y, act=act, res=res, res2=res2, out_exp=out_exp)
        if out_exp is not None:
            self._take("GELU(fc1) -> fc2", y, out_exp, self.fc2_bound[id(out_exp)])


def slack(wide):
    import math
    from patchfusion_amd import packing as pk
    from patchfusion_amd.config import make_config
    from patchfusion_amd.hip_ops import ops
    from patchfusion_amd.model import PatchFusion
    from patchfusion_amd.spec import patchfusion_spec, synthetic_state_dict
    from tests.dynamic_range import widen_dynamic_range
    dev = torch.device("cuda", 0)
    cfg = make_config("vitl", (392, 518), (2160, 3840), (4, 4))
    sd = synthetic_state_dict(patchfusion_spec(cfg), 0)
    if wide:
        sd = widen_dynamic_range(sd)
    img = torch.rand(1, 3, 2160, 3840, generator=torch.Generator().manual_seed(1234)).to(dev)
    os.environ["PF_VIT_F16X2"] = "2"                     # both branches, so that both are measured
    rec = _Recorder(ops)
    m = PatchFusion(cfg, compute_dtype="fp32", ops=rec).eval()
    m.load_state_dict(sd, strict=True)
    m = m.to(dev)
    lr = m.resizer(img)
    m._ensure_engine()
    rec.fc2_bound = {}
    for br in ("coarse", "fine"):
        net = m._engine[br]
        assert net.f16x2
        v = f"{br}_branch.core.core.pretrained.blocks."
        for i, blk in enumerate(net.blocks):
            b = f"{v}{i}."
            rec.fc2_bound[id(blk["fc2"].in_exp)] = pk.gelu_linear_bound(sd[b + "mlp.fc1.weight"], sd[b + "mlp.fc1.bias"],
                                                                        pk.layernorm_bound(sd[b + "norm2.weight"], sd[b + "norm2.bias"]))
    m(mode="infer", image_lr=lr, image_hr=img, cai_mode="m1", process_num=8)
    torch.cuda.synchronize()
    print(f"| operand ({'dynamic-range' if wide else 'synthetic'} weights) | calls | slack bits (log2 bound / observed max), min | median | 99th pct | max | channels > 12 bits |")
    print("|---|---|---|---|---|---|---|")
    for key, lst in rec.rows.items():
        s = torch.cat([torch.log2(bound.double() / mx.clamp_min(1e-300)) for mx, bound in lst]).sort().values
        q = lambda f: float(s[min(len(s) - 1, int(f * len(s)))])
        print(f"| {key} | {len(lst)} | {float(s[0]):.2f} | {q(0.5):.2f} | {q(0.99):.2f} | {float(s[-1]):.2f} | {int((s > 12).sum())} of {len(s)} |")
        assert math.isfinite(float(s[0])) and float(s[0]) >= 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("linears", "tiles", "fc2", "tile_image", "image", "slack"))
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--wide", action="store_true")
    ap.add_argument("--reverse", action="store_true", help="tile_image: build the PF_VIT_ATTN_F16X2=2 engine first")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    if a.mode == "linears":
        linears(a.rounds)
    elif a.mode == "tiles":
        tiles(a.rounds)
    elif a.mode == "fc2":
        fc2_only()
    elif a.mode == "tile_image":
        tile_image(a.steps, a.rounds, a.reverse)
    elif a.mode == "image":
        image(a.steps, a.rounds)
    else:
        slack(a.wide)


if __name__ == "__main__":
    main()
