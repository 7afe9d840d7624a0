"""GPU probe of the fp16x2 attention and projection (pf_vit_attention_f16x2, pf_gemm_f16x2) against the bf16x3 ones they replace.
usage: python tools/vit_attn_f16x2_ab.py launches [--rounds R]   attention B = 8 / 1 at S = 1037, projection at 8296 / 1037 rows and the qkv GEMM with both
                                                        store forms, old and new interleaved in one process (untimed round, then R rounds of 20
                                                        launches per route; best round)
       python tools/vit_attn_f16x2_ab.py image [--steps K] [--rounds R] [--arms 0,1] [--reverse]   whole image pass (BASELINE configs[2]), one engine
                                                        per arm (PF_VIT_ATTN_F16X2 is read at engine build; default two arms: 0 against the default),
                                                        one untimed round, then arms interleaved round by round; --reverse builds (and runs) the
                                                        arms in the opposite order; max |depth difference| against the first arm listed
       python tools/vit_attn_f16x2_ab.py slack [--wide]  log2(2^14 / observed max of x / 2^e) per channel of q, k, v and the attention output over one image
                                                        pass (fine branch); --wide: tests/dynamic_range.py weights
       python tools/vit_attn_f16x2_ab.py pass --arms V [--steps K]   one warm-up and K image passes with PF_VIT_ATTN_F16X2=V (for a kernel trace)
       python tools/vit_attn_f16x2_ab.py one attention|fc1 [--steps N]   N launches of the fp16x2 attention (B = 8, S = 1037) or of fc1 on pf_gemm_f16x2 at 8296
                                                        rows (for counter runs: tools/kernel_pmc.sh)"""
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


def _ab(name, M, arms, rounds):
    best = [1e9, 1e9]
    for rnd in range(rounds + 1):
        for i, f in enumerate(arms):
            t = _timed(f)
            if rnd:
                best[i] = min(best[i], t)
    print(f"| {name} | {M} | {best[0]:.4f} | {best[1]:.4f} | {best[0] / best[1]:.2f}x |", flush=True)


def launches(rounds):
    from patchfusion_amd import packing as pk
    from patchfusion_amd.hip_ops import ops
    g = torch.Generator().manual_seed(0)
    D, heads, S = 1024, 16, 1037
    print("| launch | rows | old ms | new ms | speed-up |")
    print("|---|---|---|---|---|")
    for B in (8, 1):
        M = B * S
        gam, bet = torch.randn(D, generator=g), torch.randn(D, generator=g) * 0.2
        bound = pk.layernorm_bound(gam, bet)
        w, b = torch.randn(3 * D, D, generator=g) / D ** 0.5, torch.randn(3 * D, generator=g)
        sc = pk.vit_attn_f16x2_scales(w, b, bound, heads).to(DEV)
        qkv = torch.randn(M, 3 * D, generator=g)
        q3 = torch.stack(pk.split3(qkv)).to(DEV)
        q2 = torch.stack(pk.split_f16x2(torch.ldexp(qkv, torch.full((3 * D,), 11.0)))).contiguous().to(DEV)        # |N(0, 1)| 2^11 < 2^14
        qk = torch.full((heads,), -22, dtype=torch.int32, device=DEV)
        o3 = torch.empty(3, D // 32, M, 32, dtype=torch.bfloat16, device=DEV)
        o2 = torch.empty(2, D // 32, M, 32, dtype=torch.float16, device=DEV)
        _ab(f"attention B = {B}, S = {S}: bf16x3 pipe vs fp16x2 pipe", M,
            [lambda: ops.vit_attention(q3, o3, B, S, heads), lambda: ops.vit_attention_f16x2(q2, o2, B, S, heads, qk)], rounds)
        ve = sc.v_exp.contiguous()
        _ab(f"attention B = {B}, S = {S}: bf16x3 pipe vs fp16x2 pipe writing three bf16 planes", M,
            [lambda: ops.vit_attention(q3, o3, B, S, heads), lambda: ops.vit_attention_f16x2(q2, o3, B, S, heads, qk, v_exp=ve)], rounds)
        wp, bp, ls = torch.randn(D, D, generator=g) / D ** 0.5, torch.randn(D, generator=g), 0.5 + torch.rand(D, generator=g)
        pw3 = pk.pack_conv_split3(wp, bp, scale=ls, kmajor=True).to(DEV)
        pw2 = pk.pack_conv_f16x2(wp, bp, ls, sc.v_bound).to(DEV)
        a3 = torch.randn(3, D // 32, M, 32, generator=g).to(torch.bfloat16).to(DEV)
        a2 = torch.randn(2, D // 32, M, 32, generator=g).to(torch.float16).to(DEV)
        x = torch.randn(M, D, generator=g).to(DEV)
        y3, y2 = torch.empty(M, D, device=DEV), torch.empty(M, D, device=DEV)
        _ab("projection 1024->1024 (+LayerScale, residual): bf16x3 vs fp16x2", M,
            [lambda: ops.conv_split3(a3, pw3, y3, res=x), lambda: ops.conv_f16x2(a2, pw2, y2, res=x)], rounds)
        pq = pk.pack_conv_f16x2(w, b, None, bound).to(DEV)
        h2 = torch.randn(2, D // 32, M, 32, generator=g).to(torch.float16).to(DEV)
        yq3 = torch.empty(3, M, 3 * D, dtype=torch.bfloat16, device=DEV)
        yq2 = torch.empty(2, M, 3 * D, dtype=torch.float16, device=DEV)
        _ab("qkv 1024->3072 fp16x2: three bf16 planes out vs two fp16 row-major planes out", M,
            [lambda: ops.conv_f16x2(h2, pq, yq3), lambda: ops.conv_f16x2(h2, pq, yq2, out_exp=sc.out_exp)], rounds)


def _setup(wide=False):
    from patchfusion_amd.config import make_config
    from patchfusion_amd.spec import patchfusion_spec, synthetic_state_dict
    cfg = make_config("vitl", (392, 518), (2160, 3840), (4, 4))
    sd = synthetic_state_dict(patchfusion_spec(cfg), 0)
    if wide:
        from tests.dynamic_range import widen_dynamic_range
        sd = widen_dynamic_range(sd)
    img = torch.rand(1, 3, 2160, 3840, generator=torch.Generator().manual_seed(1234)).to(torch.device("cuda", 0))
    return cfg, sd, img


def _engine(cfg, sd, v, dev):
    from patchfusion_amd.model import PatchFusion
    if v == "default":
        os.environ.pop("PF_VIT_ATTN_F16X2", None)
    else:
        os.environ["PF_VIT_ATTN_F16X2"] = v
    m = PatchFusion(cfg, compute_dtype="fp32").eval()
    m.load_state_dict(sd, strict=True)
    return m.to(dev)


def image(steps, rounds, arms, reverse):
    dev = torch.device("cuda", 0)
    cfg, sd, img = _setup()
    order = list(reversed(range(len(arms)))) if reverse else list(range(len(arms)))
    models = [None] * len(arms)
    for i in order:                                      # the route is fixed when the engine is built (first forward)
        m = _engine(cfg, sd, arms[i], dev)
        lr = m.resizer(img)
        m(mode="infer", image_lr=lr, image_hr=img, cai_mode="m1", process_num=8)
        torch.cuda.synchronize()
        models[i] = m
    print(f"build and run order: {[arms[i] for i in order]}; allocated with every engine resident {torch.cuda.memory_allocated() / 2 ** 20:.0f} MiB; "
          f"fine-branch routes (attn_f16x2, proj_f16x2): {[(m._engine['fine'].attn_f16x2, m._engine['fine'].proj_f16x2) for m in models]}\n", flush=True)
    assert not any(m._engine["coarse"].attn_f16x2 for m in models)
    for i in order:                                      # one untimed round
        for _ in range(steps):
            models[i](mode="infer", image_lr=lr, image_hr=img, cai_mode="m1", process_num=8)
    torch.cuda.synchronize()
    times, outs = [[] for _ in arms], [None for _ in arms]
    for r in range(rounds):
        for i in order:
            m = models[i]
            d, _ = m(mode="infer", image_lr=lr, image_hr=img, cai_mode="m1", process_num=8)
            torch.cuda.synchronize()
            outs[i] = d.clone()
            t0 = time.perf_counter()
            for _ in range(steps):
                m(mode="infer", image_lr=lr, image_hr=img, cai_mode="m1", process_num=8)
            torch.cuda.synchronize()
            times[i].append((time.perf_counter() - t0) / steps * 1e3)
            print(f"round {r} PF_VIT_ATTN_F16X2={arms[i]}: {times[i][-1]:.2f} ms", file=sys.stderr, flush=True)
    print("| variant | " + " | ".join(f"round {r} ms" for r in range(rounds)) + f" | mean ms | spread ms | vs `{arms[0]}` |")
    print("|---|" + "---|" * (rounds + 3))
    m0 = sum(times[0]) / rounds
    for i, v in enumerate(arms):
        m = sum(times[i]) / rounds
        print(f"| `PF_VIT_ATTN_F16X2={v}` | " + " | ".join(f"{t:.2f}" for t in times[i]) + f" | {m:.2f} | {max(times[i]) - min(times[i]):.2f} | {m - m0:+.2f} |")
    spread = max(max(t) - min(t) for t in times)
    for i in range(1, len(arms)):
        gain = m0 - sum(times[i]) / rounds
        print(f"\n`{arms[i]}` against `{arms[0]}`: gain {gain:.2f} ms, larger within-arm spread {spread:.2f} ms, ratio {gain / spread:.1f} (rule: >= 3); "
              f"max |depth difference| {float((outs[i] - outs[0]).abs().max()):.3e} (depth max {float(outs[0].abs().max()):.3f})")
    print(f"\n{steps} images per cell, split 4x4, process_num 8")


def one_pass(steps, arm):
    dev = torch.device("cuda", 0)
    cfg, sd, img = _setup()
    m = _engine(cfg, sd, arm, dev)
    lr = m.resizer(img)
    for _ in range(steps + 1):
        m(mode="infer", image_lr=lr, image_hr=img, cai_mode="m1", process_num=8)
    torch.cuda.synchronize()
    print(f"PF_VIT_ATTN_F16X2={arm}: 1 + {steps} image passes; fine branch attn_f16x2 = {m._engine['fine'].attn_f16x2}, proj_f16x2 = {m._engine['fine'].proj_f16x2}")


def one(which, n):
    from patchfusion_amd import packing as pk
    from patchfusion_amd.hip_ops import ops
    g = torch.Generator().manual_seed(0)
    D, heads, S, B = 1024, 16, 1037, 8
    M = B * S
    if which == "attention":
        q2 = torch.stack(pk.split_f16x2(torch.ldexp(torch.randn(M, 3 * D, generator=g), torch.full((3 * D,), 11.0)))).contiguous().to(DEV)
        qk = torch.full((heads,), -22, dtype=torch.int32, device=DEV)
        o2 = torch.empty(2, D // 32, M, 32, dtype=torch.float16, device=DEV)
        fn = lambda: ops.vit_attention_f16x2(q2, o2, B, S, heads, qk)
    else:
        bound = pk.layernorm_bound(torch.randn(D, generator=g), torch.randn(D, generator=g) * 0.2)
        w, b = torch.randn(4 * D, D, generator=g) / D ** 0.5, torch.randn(4 * D, generator=g)
        pw = pk.pack_conv_f16x2(w, b, None, bound).to(DEV)
        h2 = torch.randn(2, D // 32, M, 32, generator=g).to(torch.float16).to(DEV)
        y2 = torch.empty(2, 4 * D // 32, M, 32, dtype=torch.float16, device=DEV)
        oe = pk.bound_exponents(pk.gelu_linear_bound(w, b, bound)).to(DEV)
        fn = lambda: ops.conv_f16x2(h2, pw, y2, act="gelu", out_exp=oe)
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    print(f"{n} launches of {which}")


class _Recorder:
    """the HIP op set, with q / k / v and the attention output read back after each call: per channel max |value| against 2^(exponent + 14)"""

    def __init__(self, ops):
        self._ops, self.rows = ops, {}

    def __getattr__(self, k):
        return getattr(self._ops, k)

    def conv_f16x2(self, x2, pw, y, act=None, res=None, res2=None, out_exp=None):
        self._ops.conv_f16x2(x2, pw, y, act=act, res=res, res2=res2, out_exp=out_exp)
        if out_exp is not None and y.dim() == 3:
            mx = y.float().sum(0).abs().amax(0).cpu()                       # in units of 2^e
            D = mx.numel() // 3
            for i, n in enumerate("qkv"):
                self.rows.setdefault(n, []).append(mx[i * D:(i + 1) * D])

    def vit_attention_f16x2(self, qkv2, out2, B, S, heads, qk_exp, v_exp=None):
        self._ops.vit_attention_f16x2(qkv2, out2, B, S, heads, qk_exp, v_exp=v_exp)
        mx = out2.float().sum(0).abs().amax(1).reshape(-1)                   # [D] per channel
        if v_exp is not None:                                               # three bf16 planes of the output itself: back to units of 2^ev
            mx = torch.ldexp(mx, -v_exp.float())
        self.rows.setdefault("attention output", []).append(mx.cpu())


def slack(wide):
    from patchfusion_amd.hip_ops import ops
    from patchfusion_amd.model import PatchFusion
    dev = torch.device("cuda", 0)
    cfg, sd, img = _setup(wide)
    rec = _Recorder(ops)
    m = PatchFusion(cfg, compute_dtype="fp32", ops=rec).eval()
    m.load_state_dict(sd, strict=True)
    m = m.to(dev)
    lr = m.resizer(img)
    m(mode="infer", image_lr=lr, image_hr=img, cai_mode="m1", process_num=8)
    torch.cuda.synchronize()
    assert m._engine["fine"].attn_f16x2
    print(f"| operand ({'dynamic-range' if wide else 'synthetic'} weights) | calls | slack bits log2(2^14 / observed max of x / 2^e), min | median | 99th pct | max | channels > 17 bits |")
    print("|---|---|---|---|---|---|---|")
    for key, lst in rec.rows.items():
        s = torch.cat([14.0 - torch.log2(mx.double().clamp_min(1e-300)) for mx in lst]).sort().values
        q = lambda f: float(s[min(len(s) - 1, int(f * len(s)))])
        print(f"| {key} | {len(lst)} | {float(s[0]):.2f} | {q(0.5):.2f} | {q(0.99):.2f} | {float(s[-1]):.2f} | {int((s > 17).sum())} of {len(s)} |")
        assert float(s[0]) >= 0, "an operand exceeded its static bound"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("launches", "image", "slack", "pass", "one"))
    ap.add_argument("what", nargs="?", default="attention", choices=("attention", "fc1"))
    ap.add_argument("--arms", default="0,default")
    ap.add_argument("--reverse", action="store_true")
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--wide", action="store_true")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    if a.mode == "launches":
        launches(a.rounds)
    elif a.mode == "image":
        image(a.steps, a.rounds, a.arms.split(","), a.reverse)
    elif a.mode == "pass":
        one_pass(a.steps, a.arms.split(",")[0])
    elif a.mode == "one":
        one(a.what, a.steps)
    else:
        slack(a.wide)


if __name__ == "__main__":
    main()
