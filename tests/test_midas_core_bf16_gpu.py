"""The bf16 mode of the native MiDaS DPT_BEiT_L_384 core on the MI355X, against float64 (tests/midas_beit_ref.py run in float64 on the GPU).
The yardstick of every bar is what PyTorch makes of the same computation in torch.bfloat16 (a user calling .bfloat16() on the restatement):
the HIP error against float64 may be at most 2x that comparator's normwise and at the 99.9th percentile, 4x on the single largest element (an
extreme-value statistic; the margins of tests/test_midas_core_gpu.py).
  * the biased bf16 attention alone (B = 1, 3; 24 x 32 and 10 x 14, both ending in a partial query block); the bias is really applied; with an
    all-zero table the output equals the unbiased bf16 attention's within one bf16 ulp everywhere;
  * the two bf16 helpers: bit-exact round-to-nearest-even of the float32 kernel's rows / exact copies;
  * the whole core, full depth, B = 1 and 3, per map, with the float32 HIP core's error printed beside the two;
  * end to end against the oracle fed by the float64 restatement: max |d| <= 2 E_core + 1e-2;
  * configs[4]'s schedule in bf16 with native cores, timed against the float32 run in the same process (alternating).

Measured on the MI355X (max / p99.9 / normwise; the full per-map table is in DESIGN.md 10, the run in profiles/r11_midas_core_bf16_gpu.log):
  attention 24 x 32, B = 1: HIP 1.54e-2 / 4.20e-3 / 1.82e-3, torch.bfloat16 9.39e-2 / 3.52e-2 / 1.32e-2; zero table: bit-identical to the unbiased kernel
  whole core B = 1 (bfloat16 restatement on the GPU): rel_depth HIP bf16 2.03 / 1.46 / 1.31e-2, bfloat16 restatement 2.30 / 1.91 / 2.23e-2, HIP fp32
    4.66e-4 / 3.62e-4 / 2.96e-6; the six maps 1.05e-2 .. 1.22e-2 normwise against 1.29e-2 .. 1.40e-2; worst max ratio r1 at B = 1, 3.44 against 3.22
  whole core B = 3: rel_depth 2.38 / 1.79 / 1.48e-2 against 2.71 / 1.90 / 1.70e-2; maps 1.02e-2 .. 1.22e-2 against 1.21e-2 .. 1.36e-2 normwise
  end to end: max |d| 2.92e-2, p99 5.19e-3, mean 1.08e-3, std(ref) 2.35e-2; E_core 3.77e-2, bar 8.54e-2
  configs[4]: bf16 0.873 / 0.877 s per image, fp32 1.570 / 1.567 s (alternating), peak 27.1 GiB with both models resident"""
import copy
import math
import random
import time

import pytest
import torch

from tests import midas_beit_ref as mb

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16


def _ops():
    from patchfusion_amd.hip_ops import ops
    return ops


def _stats(got, ref64):
    """(max, p99.9, normwise) error against the float64 reference"""
    d = (got.double() - ref64).abs().flatten()
    return float(d.max()), float(d.kthvalue(max(1, int(0.999 * d.numel()))).values), float(d.norm() / ref64.norm())


def _within(e, c):
    return e[2] <= 2 * c[2] and e[1] <= 2 * c[1] and e[0] <= 4 * c[0]


def _ulp_bf16(x):
    """one bf16 unit in the last place at |x| (8 significand bits; the smallest normal's below it)"""
    e = torch.floor(torch.log2(x.abs().float().clamp_min(2.0 ** -126)))
    return torch.exp2(e - 7)


@pytest.mark.parametrize("grid", [(24, 32), (10, 14)])
@pytest.mark.parametrize("B", [1, 3])
def test_bf16_rpb_attention_against_float64(B, grid):
    ops = _ops()
    th, tw = grid
    Hh = 16
    S, D = th * tw + 1, Hh * 64
    assert S % 128 != 0                                               # the last query block is partial
    g = torch.Generator(device=DEV).manual_seed(100 * B + th)
    qkv = (torch.randn(B * S, 3 * D, device=DEV, generator=g) * 1.5).to(BF)       # bf16 values: q / 8 is exact in bf16 too
    x = qkv.double()
    tab = torch.randn(47 * 47 + 3, Hh, device=DEV, generator=g)       # unit standard deviation: the bias matters
    from patchfusion_amd import packing as pk
    tab2 = pk.beit_rel_pos_table(tab, 24, th, tw).to(DEV)
    out = torch.full((B * S, D), float("nan"), dtype=BF, device=DEV)
    ops.vit_attention_rpb_bf16(qkv, out, B, S, Hh, tab2, th, tw)
    torch.cuda.synchronize()
    got = out.view(B, S, Hh, 64)

    def attn(xx, bias):
        q, k, v = xx.view(B, S, 3, Hh, 64).permute(2, 0, 3, 1, 4).unbind(0)
        a = (q * 0.125) @ k.transpose(-2, -1) + bias
        return (a.softmax(-1) @ v).transpose(1, 2)
    bias64 = (tab2.double() / math.log2(math.e)).t()[mb.gen_relative_position_index(th, tw).to(DEV).view(-1)].view(S, S, Hh).permute(2, 0, 1)
    ref = attn(x, bias64)
    cmp = attn(qkv, bias64.to(BF))                                    # PyTorch in torch.bfloat16 on the same operands
    e, c = _stats(got, ref), _stats(cmp, ref)
    print(f"\nbf16 rpb attention B={B} {th}x{tw}: hip max {e[0]:.3e} p99.9 {e[1]:.3e} norm {e[2]:.3e} | torch.bfloat16 max {c[0]:.3e} p99.9 {c[1]:.3e} norm {c[2]:.3e}")
    assert torch.isfinite(got.float()).all()
    assert _within(e, c), (e, c)
    # with the bias zeroed in the reference the result is far outside that bound: the bias is really applied
    nb = _stats(got, attn(x, torch.zeros_like(bias64)))
    print(f"  against the reference WITHOUT bias: norm {nb[2]:.3e}")
    assert nb[2] > 10 * 2 * c[2], (nb, c)
    # an all-zero table: the unbiased bf16 attention's output within one bf16 ulp on every element
    plain = torch.empty_like(out)
    ops.vit_attention(qkv, plain, B, S, Hh)
    zero = torch.full_like(out, float("nan"))
    ops.vit_attention_rpb_bf16(qkv, zero, B, S, Hh, torch.zeros_like(tab2), th, tw)
    torch.cuda.synchronize()
    diff = (zero.float() - plain.float()).abs()
    ulp = torch.maximum(_ulp_bf16(zero), _ulp_bf16(plain))
    print(f"  zero table vs unbiased kernel: bit-identical = {torch.equal(zero, plain)}, max |d| / ulp = {float((diff / ulp).max()):.2f}")
    assert bool((diff <= ulp).all())


def test_bf16_attention_refusals():
    ops = _ops()
    qkv = torch.zeros(141, 3 * 64, dtype=BF, device=DEV)
    out = torch.zeros(141, 64, dtype=BF, device=DEV)
    tab = torch.zeros(1, 19 * 27 + 3, device=DEV)
    ops.vit_attention_rpb_bf16(qkv, out, 1, 141, 1, tab, 10, 14)
    with pytest.raises(ValueError):
        ops.vit_attention_rpb_bf16(qkv, out, 1, 141, 1, tab, 7, 20)              # table of another grid
    with pytest.raises(ValueError):
        ops.vit_attention_rpb_bf16(qkv.float(), out, 1, 141, 1, tab, 10, 14)
    with pytest.raises(ValueError):
        ops.vit_attention_rpb_bf16(qkv, out, 1, 141, 1, tab.to(BF), 10, 14)


def test_bf16_helpers_are_roundings_and_copies():
    ops = _ops()
    img = torch.rand(2, 3, 64, 96, device=DEV)
    c32 = torch.full((2 * 4 * 6, 776), float("nan"), device=DEV)
    c16 = torch.full((2 * 4 * 6, 776), float("nan"), dtype=BF, device=DEV)
    ops.patch_im2col_norm(img, c32, 16, (0.5, 0.5, 0.5), (0.5, 0.5, 0.5))
    ops.patch_im2col_norm(img, c16, 16, (0.5, 0.5, 0.5), (0.5, 0.5, 0.5))
    assert torch.equal(c16, c32.to(BF))                               # round to nearest even of the float32 rows, bit for bit
    assert float(c16[:, 768:].float().abs().max()) == 0.0
    x = torch.randn(3 * 769, 1024, device=DEV).to(BF)
    y = torch.full((3 * 768, 2048), float("nan"), dtype=BF, device=DEV)
    ops.readout_concat(x, y, 3, 769)
    xv = x.view(3, 769, 1024)
    want = torch.cat((xv[:, 1:], xv[:, :1].expand(-1, 768, -1)), -1).reshape(3 * 768, 2048)
    assert torch.equal(y, want)
    with pytest.raises(ValueError):
        ops.readout_concat(x, y.float(), 3, 769)


@pytest.fixture(scope="module")
def full_core():
    from patchfusion_amd.midas_core import MidasBeitCore
    ref = mb.seeded(mb.settings(), seed=11, dtype=torch.float64).to(DEV)
    sd = {"core." + k: v for k, v in ref.state_dict().items()}
    c32 = MidasBeitCore("DPT_BEiT_L_384").load_state_dict(sd)
    c16 = MidasBeitCore("DPT_BEiT_L_384").load_state_dict(sd)
    c16.call_dtype = BF
    return ref, c32, c16


def _bf16_restatement(ref):
    """the restatement cast to bfloat16 and the device it runs on: the GPU if PyTorch's operators take bfloat16 there, else the CPU"""
    r16 = copy.deepcopy(ref).bfloat16()
    try:
        with torch.no_grad():
            r16.provider(torch.rand(1, 3, 384, 512, device=DEV))
        torch.cuda.synchronize()
        return r16, DEV
    except RuntimeError as e:
        print(f"\n(bfloat16 restatement on the CPU: {str(e)[:120]})")
        return r16.cpu(), "cpu"


@pytest.mark.parametrize("B", [1, 3])
def test_whole_bf16_core_against_float64_restatement(full_core, B):
    ref, c32, c16 = full_core
    img = torch.rand(B, 3, 384, 512, device=DEV, generator=torch.Generator(device=DEV).manual_seed(20 + B))
    r16m, where = _bf16_restatement(ref)
    with torch.no_grad():
        r64, f64 = ref.provider(img.double())
        ra, fa = r16m.provider(img.to(where))
        rh, fh = c16(img)
        r32, f32 = c32(img)
    assert c16._packed["dtype"] == BF and c32._packed["dtype"] == torch.float32
    names = ["rel_depth", "l4_rn", "r4", "r3", "r2", "r1", "out_conv"]
    print(f"\nwhole bf16 core B={B} (bfloat16 restatement on {where}); max / p99.9 / norm against the float64 restatement")
    bad = []
    for n, h, a, s, w in zip(names, [rh] + fh, [ra] + fa, [r32] + f32, [r64] + f64):
        assert h.shape == w.shape and h.dtype == torch.float32, (n, h.shape, w.shape, h.dtype)
        eh, ea, es = _stats(h, w), _stats(a.to(DEV), w), _stats(s, w)
        print(f"  {n:9s} hip bf16 {eh[0]:.3e} {eh[1]:.3e} {eh[2]:.3e} | bfloat16 restatement {ea[0]:.3e} {ea[1]:.3e} {ea[2]:.3e} | hip fp32 {es[0]:.3e} {es[1]:.3e} {es[2]:.3e}")
        assert torch.isfinite(h).all()
        if not _within(eh, ea):
            bad.append((n, eh, ea))
    assert not bad, bad


def _zoe_model(cfg, dtype, core_sd):
    from patchfusion_amd.model import PatchFusion
    from patchfusion_amd.spec import patchfusion_spec, synthetic_state_dict
    sd = synthetic_state_dict(patchfusion_spec(cfg), 0)
    m = PatchFusion(cfg, compute_dtype=dtype, core_providers="native").eval()
    m.load_state_dict(sd, strict=True)
    for p in m.core_providers:
        p.load_state_dict(core_sd)
    return m.to(DEV), sd


def test_end_to_end_bf16_native_cores_against_oracle(full_core):
    """make_zoe_config((384, 512), (1536, 2048), (2, 2)), r4, process_num = 2, bf16, native cores, against pf_oracle.Oracle fed by the float64
    restatement.  Bar: max |d| <= 2 E_core + 1e-2, E_core = max difference between the oracle fed by the bfloat16-cast restatement and the
    oracle fed by the float64 one (the reference-side cost of a bf16 core), 1e-2 = the project's bar for everything after the core in bf16 at
    this geometry (tests/test_e2e_gpu.py test_zoe_midas_core_geometry_r_mode_vs_oracle)."""
    from oracle import pf_oracle
    from patchfusion_amd.config import make_zoe_config
    ref = full_core[0]
    cfg = make_zoe_config((384, 512), (1536, 2048), (2, 2))
    core_sd = {"core." + k: v for k, v in ref.state_dict().items()}
    m, sd = _zoe_model(cfg, "bf16", core_sd)
    r16m, where = _bf16_restatement(ref)

    def restated(img):
        rel, feats = ref.provider(img.to(DEV, torch.float64))
        return rel.float().cpu(), [f.float().cpu() for f in feats]

    def restated16(img):
        rel, feats = r16m.provider(img.to(where))
        return rel.float().cpu(), [f.float().cpu() for f in feats]

    img = torch.rand(1, 3, 1536, 2048, generator=torch.Generator().manual_seed(1234))
    lr = m.resizer(img)
    random.seed(5621)
    with torch.no_grad():
        d, _ = m(mode="infer", image_lr=lr.to(DEV), image_hr=img.to(DEV), cai_mode="r4", process_num=2)
    random.seed(5621)
    with torch.no_grad():
        want = pf_oracle.Oracle(cfg, sd, core_providers=(restated, restated)).infer(lr, img, "r4", 2)
    random.seed(5621)
    with torch.no_grad():
        want16 = pf_oracle.Oracle(cfg, sd, core_providers=(restated16, restated16)).infer(lr, img, "r4", 2)
    e_core = float((want16 - want).abs().max())
    dd = (d.float().cpu() - want).abs().flatten()
    err, p99, mean = float(dd.max()), float(dd.kthvalue(int(0.99 * dd.numel())).values), float(dd.mean())
    print(f"\nend to end bf16 (native cores vs oracle + float64 restatement): max |d| = {err:.3e} p99 {p99:.3e} mean {mean:.3e}; "
          f"E_core (oracle + bfloat16 restatement on {where}) = {e_core:.3e}; bar {2 * e_core + 1e-2:.3e}; std(ref) {float(want.std()):.3e}")
    assert d.shape == want.shape and torch.isfinite(d).all()
    assert float(want.std()) > 1e-3
    assert err <= 2 * e_core + 1e-2, (err, e_core)


def test_configs4_schedule_bf16_with_native_cores(full_core):
    from patchfusion_amd.config import make_zoe_config
    ref = full_core[0]
    cfg = make_zoe_config()
    core_sd = {"core." + k: v for k, v in ref.state_dict().items()}
    models = {dt: _zoe_model(cfg, dt, core_sd)[0] for dt in ("fp32", "bf16")}
    img = torch.rand(1, 3, 2160, 3840, generator=torch.Generator().manual_seed(7))
    lr, hr = models["bf16"].resizer(img).to(DEV), img.to(DEV)

    def run(dt):
        random.seed(0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with torch.no_grad():
            d, _ = models[dt](mode="infer", image_lr=lr, image_hr=hr, cai_mode="r128", process_num=4)
        torch.cuda.synchronize()
        return d, time.perf_counter() - t0
    for dt in ("fp32", "bf16"):                                        # one warm-up each
        run(dt)
    torch.cuda.reset_peak_memory_stats()
    t = {"fp32": [], "bf16": []}
    for dt in ("fp32", "bf16", "fp32", "bf16"):
        d, s = run(dt)
        t[dt].append(s)
        if dt == "bf16":
            peak = torch.cuda.max_memory_allocated() / 2 ** 30
    print(f"\nconfigs[4] (2160x3840, 4x4 + r128 = 177 patches, native cores): bf16 {t['bf16'][0]:.3f} / {t['bf16'][1]:.3f} s per image, "
          f"fp32 {t['fp32'][0]:.3f} / {t['fp32'][1]:.3f} s per image (alternating, both models resident), peak {peak:.2f} GiB")
    assert tuple(d.shape[-2:]) == (2160, 3840) and torch.isfinite(d).all()
    assert float(d.min()) >= cfg["min_depth"] and float(d.max()) <= cfg["max_depth"]
    # a fast mode slower than the exact mode is a defect: not slower than float32 by more than the spread of the float32 runs
    spread = abs(t["fp32"][0] - t["fp32"][1])
    assert min(t["bf16"]) <= min(t["fp32"]) + spread, t
