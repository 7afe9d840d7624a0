"""The native MiDaS DPT_BEiT_L_384 core on the MI355X, against float64 (tests/midas_beit_ref.py run in float64 on the GPU):
  * the relative-position attention (S = 769, 16 heads, wide tables), the 16x16 normalised im2col and the readout rows;
  * the whole core at full depth, B = 1 and 3: on rel_depth and each of the six maps the HIP error is at most 2x the float32 restatement's
    (normwise and at p99.9; 4x on the single largest element);
  * end to end: PatchFusion with native cores against the oracle with the float64 restatement as its providers (2e-5);
  * configs[4]'s schedule (2160x3840, 4x4 + r128 = 177 patches) with native cores: finite, right shape; time and peak memory printed."""
import copy
import math
import random
import time

import pytest
import torch

from tests import midas_beit_ref as mb

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _ops():
    from patchfusion_amd.hip_ops import ops
    return ops


def _errs(got, ref64):
    d = (got.double() - ref64).abs()
    return float(d.max()), float(d.norm() / ref64.norm())


def _p999(got, ref64):
    d = (got.double() - ref64).abs().flatten()
    return float(d.kthvalue(max(1, int(0.999 * d.numel()))).values)


@pytest.mark.parametrize("qw", [16, 32])
@pytest.mark.parametrize("B", [1, 3])
def test_rpb_attention_against_float64(B, qw, monkeypatch):
    monkeypatch.setenv("PF_ATTN_QW", str(qw))         # both instantiations: 16 and 32 queries per wave (different table slices per block)
    ops = _ops()
    th, tw, Hh = 24, 32, 16
    S, D = th * tw + 1, Hh * 64
    g = torch.Generator(device=DEV).manual_seed(B)
    qkv = torch.randn(B * S, 3 * D, device=DEV, generator=g) * 1.5
    qkv3 = torch.empty((3, B * S, 3 * D), dtype=torch.bfloat16, device=DEV)
    ops.split3(qkv, qkv3)
    x = qkv3.double().sum(0)                                      # the exact operand values the kernel sees
    tab = torch.randn(47 * 47 + 3, Hh, device=DEV, generator=g)    # std 1: the bias matters
    from patchfusion_amd import packing as pk
    tab2 = pk.beit_rel_pos_table(tab, 24, th, tw).to(DEV)
    out = torch.full((3, B * S, D), float("nan"), dtype=torch.bfloat16, device=DEV)
    ops.vit_attention_rpb(qkv3, out, B, S, Hh, tab2, th, tw)
    torch.cuda.synchronize()
    got = out.double().sum(0).view(B, S, Hh, 64)

    def attn(xx, bias):
        q, k, v = xx.view(B, S, 3, Hh, 64).permute(2, 0, 3, 1, 4).unbind(0)
        a = (q * 0.125) @ k.transpose(-2, -1) + bias
        return (a.softmax(-1) @ v).transpose(1, 2)
    bias64 = (tab2.double() / math.log2(math.e)).t()[mb.gen_relative_position_index(th, tw).to(DEV).view(-1)].view(S, S, Hh).permute(2, 0, 1)
    ref = attn(x, bias64)
    f32 = attn(x.float(), bias64.float())
    e_gpu, e_f32 = _errs(got, ref), _errs(f32, ref)
    print(f"\nrpb attention B={B} qw={qw}: hip max {e_gpu[0]:.3e} norm {e_gpu[1]:.3e} | float32 max {e_f32[0]:.3e} norm {e_f32[1]:.3e}")
    assert torch.isfinite(got).all()
    assert e_gpu[0] <= 2 * e_f32[0] and e_gpu[1] <= 2 * e_f32[1], (e_gpu, e_f32)
    # without the bias the output is far away: the bias is really applied
    assert _errs(got, attn(x, torch.zeros_like(bias64)))[0] > 100 * e_f32[0]


def test_im2col_norm_and_readout_against_float64():
    ops = _ops()
    img = torch.rand(2, 3, 64, 96, device=DEV)
    col = torch.full((2 * 4 * 6, 776), float("nan"), device=DEV)
    ops.patch_im2col_norm(img, col, 16, (0.5, 0.5, 0.5), (0.5, 0.5, 0.5))
    ref = ((img.double() - 0.5) / 0.5).unfold(2, 16, 16).unfold(3, 16, 16)          # [B,3,ty,tx,ky,kx]
    ref = ref.permute(0, 2, 3, 4, 5, 1).reshape(2 * 24, 768)
    assert float((col[:, :768].double() - ref).abs().max()) <= 2 ** -23 * 2
    assert float(col[:, 768:].abs().max()) == 0.0
    x = torch.randn(3 * 769, 1024, device=DEV)
    y = torch.full((3 * 768, 2048), float("nan"), device=DEV)
    ops.readout_concat(x, y, 3, 769)
    xv = x.view(3, 769, 1024)
    want = torch.cat((xv[:, 1:], xv[:, :1].expand(-1, 768, -1)), -1).reshape(3 * 768, 2048)
    assert torch.equal(y, want)


@pytest.fixture(scope="module")
def full_core():
    from patchfusion_amd.midas_core import MidasBeitCore
    ref = mb.seeded(mb.settings(), seed=11, dtype=torch.float64).to(DEV)
    core = MidasBeitCore("DPT_BEiT_L_384").load_state_dict({"core." + k: v for k, v in ref.state_dict().items()})
    return ref, core


@pytest.mark.parametrize("B", [1, 3])
def test_whole_core_against_float64_restatement(full_core, B):
    ref, core = full_core
    img = torch.rand(B, 3, 384, 512, device=DEV, generator=torch.Generator(device=DEV).manual_seed(20 + B))
    with torch.no_grad():
        r64, f64 = ref.provider(img.double())
        r32, f32 = copy.deepcopy(ref).float().provider(img)
        rh, fh = core(img)
    names = ["rel_depth", "l4_rn", "r4", "r3", "r2", "r1", "out_conv"]
    print(f"\nwhole core B={B}")
    for n, h, a, w in zip(names, [rh] + fh, [r32] + f32, [r64] + f64):
        assert h.shape == w.shape, (n, h.shape, w.shape)
        eh, ea = _errs(h, w), _errs(a, w)
        ph, pa = _p999(h, w), _p999(a, w)
        print(f"  {n:9s} hip max {eh[0]:.3e} p99.9 {ph:.3e} norm {eh[1]:.3e} | float32 restatement max {ea[0]:.3e} p99.9 {pa:.3e} norm {ea[1]:.3e}")
        assert torch.isfinite(h).all()
        # norm-wise and at the 99.9th percentile within 2x of float32; the single largest element within 4x -- a LOOSER bar than 2x (DESIGN
        # §10): it is an extreme-value statistic of ~10^5-10^6 samples, and the float32 restatement's own max moves 2.4x between B = 1 and
        # B = 3 on l4_rn (measured B = 1 ratio 2.64x)
        assert eh[1] <= 2 * ea[1] and ph <= 2 * pa and eh[0] <= 4 * ea[0], (n, eh, ea, ph, pa)


def test_configs4_schedule_with_native_cores(full_core):
    from patchfusion_amd.config import make_zoe_config
    from patchfusion_amd.model import PatchFusion
    from patchfusion_amd.spec import patchfusion_spec, synthetic_state_dict
    ref, _ = full_core
    cfg = make_zoe_config()
    sd = synthetic_state_dict(patchfusion_spec(cfg), 0)
    m = PatchFusion(cfg, compute_dtype="fp32", core_providers="native").eval()
    m.load_state_dict(sd, strict=True)
    core_sd = {"core." + k: v for k, v in ref.state_dict().items()}
    for p in m.core_providers:
        p.load_state_dict(core_sd)
    m = m.to(DEV)
    img = torch.rand(1, 3, 2160, 3840, generator=torch.Generator().manual_seed(7))
    lr = m.resizer(img)
    random.seed(0)
    torch.cuda.reset_peak_memory_stats()
    with torch.no_grad():
        d, _ = m(mode="infer", image_lr=lr.to(DEV), image_hr=img.to(DEV), cai_mode="r128", process_num=4)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        random.seed(0)
        d, _ = m(mode="infer", image_lr=lr.to(DEV), image_hr=img.to(DEV), cai_mode="r128", process_num=4)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
    print(f"\nconfigs[4] (2160x3840, 4x4 + r128 = 177 patches, native cores): {dt:.3f} s per image, peak {torch.cuda.max_memory_allocated() / 2**30:.2f} GiB")
    assert tuple(d.shape[-2:]) == (2160, 3840) and torch.isfinite(d).all()


def test_end_to_end_native_cores_against_oracle(full_core):
    """make_zoe_config((384, 512), (1536, 2048), (2, 2)), r4: the engine with native cores against pf_oracle.Oracle with the float64
    restatement (run on the GPU, results handed back as float32 on the CPU) as both providers, on the same weights; final map within 2e-5"""
    from oracle import pf_oracle
    from patchfusion_amd.config import make_zoe_config
    from patchfusion_amd.model import PatchFusion
    from patchfusion_amd.spec import patchfusion_spec, synthetic_state_dict
    ref, _ = full_core
    cfg = make_zoe_config((384, 512), (1536, 2048), (2, 2))
    sd = synthetic_state_dict(patchfusion_spec(cfg), 0)

    def restated(img):
        rel, feats = ref.provider(img.to(DEV, torch.float64))
        return rel.float().cpu(), [f.float().cpu() for f in feats]

    m = PatchFusion(cfg, compute_dtype="fp32", core_providers="native").eval()
    m.load_state_dict(sd, strict=True)
    core_sd = {"core." + k: v for k, v in ref.state_dict().items()}
    for p in m.core_providers:
        p.load_state_dict(core_sd)
    m = m.to(DEV)
    img = torch.rand(1, 3, 1536, 2048, generator=torch.Generator().manual_seed(1234))
    lr = m.resizer(img)
    random.seed(5621)
    with torch.no_grad():
        d, _ = m(mode="infer", image_lr=lr.to(DEV), image_hr=img.to(DEV), cai_mode="r4", process_num=2)
    random.seed(5621)
    with torch.no_grad():
        want = pf_oracle.Oracle(cfg, sd, core_providers=(restated, restated)).infer(lr, img, "r4", 2)
    err = float((d.cpu() - want).abs().max())
    print(f"\nend to end (native cores vs oracle + float64 restatement): max |d| = {err:.3e}, map std {float(want.std()):.3e}")
    assert d.shape == want.shape and err <= 2e-5, err
    assert float(want.std()) > 1e-3
