"""pytest -m gpu: the fp16x2 attention (csrc/attn_split3.hip pf_vit_attention_f16x2), the fp16x2 projection and the row-major fp16x2 store form of the
qkv GEMM (pf_gemm_f16x2, korder bit 32), each alone, from cold caches, against float64 -- next to the bf16x3 kernels they replace on the SAME float32
inputs.

Inputs: random ViT-L-shaped weights (LayerNorm, qkv 1024 -> 3072, projection 1024 -> 1024 with LayerScale), once as drawn and once through
tests/dynamic_range.py (q channel c x s_c, k channel c / s_c, v channel c x t_c, projection input column c / t_c; s, t over six decades).  Cases
B = 8 and B = 1 at S = 1037.  Bar (the rule round 9 set for every split route): the error of the new route is at most TWICE the error of the
existing bf16x3 kernel measured in the same test, normwise (max |y - ref| / max |ref|) and element-wise in the sense of tests/f64_ref.py
(max |y - ref| / mag, mag = the sum of the magnitudes of the terms of that element).  Two launches are bit-identical; NaN / inf in -> non-finite out."""
import pytest
import torch

from patchfusion_amd import packing as pk
from patchfusion_amd.hip_ops import ops
from tests import f64_ref, op_checks
from tests.dynamic_range import widen_dynamic_range

pytestmark = pytest.mark.gpu
DEV = "cuda"
D, HEADS, S = 1024, 16, 1037
TINY = f64_ref.TINY


def _weights(wide):
    g = torch.Generator().manual_seed(21)
    sd = {"x.pretrained.blocks.0.norm1.weight": 1.0 + 0.3 * torch.randn(D, generator=g), "x.pretrained.blocks.0.norm1.bias": 0.2 * torch.randn(D, generator=g),
          "x.pretrained.blocks.0.attn.qkv.weight": torch.randn(3 * D, D, generator=g) / D ** 0.5,
          "x.pretrained.blocks.0.attn.qkv.bias": 0.5 * torch.randn(3 * D, generator=g),
          "x.pretrained.blocks.0.attn.proj.weight": torch.randn(D, D, generator=g) / D ** 0.5,
          "x.pretrained.blocks.0.attn.proj.bias": 0.5 * torch.randn(D, generator=g),
          "x.pretrained.blocks.0.ls1.gamma": 0.5 + torch.rand(D, generator=g)}
    if wide:
        sd = widen_dynamic_range(sd, seed=3)
    return {k.split("blocks.0.")[1]: v.float() for k, v in sd.items()}


def _case(B, wide):
    """float32 LayerNorm output h, qkv = float32(h W^T + b) (the operand both attention routes receive), weights, static scales"""
    w = _weights(wide)
    g = torch.Generator().manual_seed(100 + B)
    x = (torch.randn(B * S, D, generator=g) * (0.5 + torch.rand(D, generator=g)) + torch.randn(D, generator=g)).float()
    h = torch.nn.functional.layer_norm(x.double(), (D,), w["norm1.weight"].double(), w["norm1.bias"].double(), 1e-6)
    qkv = (h.to(DEV) @ w["attn.qkv.weight"].double().t().to(DEV) + w["attn.qkv.bias"].double().to(DEV)).float()
    bn1 = pk.layernorm_bound(w["norm1.weight"], w["norm1.bias"])
    sc = pk.vit_attn_f16x2_scales(w["attn.qkv.weight"], w["attn.qkv.bias"], bn1, HEADS)
    return w, x, h.float(), qkv, bn1, sc


def _attn64(qkv, B):
    """float64 attention on the float32 qkv (on the device, torch's own float64 kernels) -> (ref, mag) [B*S, D]: mag = sum_j p_ij |v_jd|"""
    q, k, v = qkv.double().view(B, S, 3, HEADS, 64).permute(2, 0, 3, 1, 4)
    p = ((q * 0.125) @ k.transpose(-2, -1)).softmax(-1)
    back = lambda t: t.transpose(1, 2).reshape(B * S, D).cpu()
    return back(p @ v), back(p @ v.abs())


def _planes2_rows(t, exp):
    """float32 [M, N] -> two fp16 planes [2, M, N] of t / 2^exp (host split; what the qkv GEMM's epilogue computes per element)"""
    return torch.stack(pk.split_f16x2(torch.ldexp(t.cpu().double(), -exp.cpu().double()[None, :]).float())).contiguous()


def _errs(y, ref, mag):
    y = y.double().cpu()
    if not torch.isfinite(y).all():
        return float("inf"), float("inf")
    d = (y - ref).abs()
    return float((d / (mag + TINY)).max()), float(d.max() / ref.abs().max())


def _kmaj2_rows(y2, exp):
    return torch.ldexp(pk.kmajor_to_rows(y2.cpu()).double().sum(0), exp.cpu().double()[None, :])


@pytest.mark.parametrize("wide", [False, True], ids=["plain", "dynamic_range"])
@pytest.mark.parametrize("B", [8, 1])
def test_attention_matches_float64_within_twice_bf16x3(B, wide):
    w, x, h, qkv, bn1, sc = _case(B, wide)
    ref, mag = _attn64(qkv, B)
    M = B * S
    q2 = _planes2_rows(qkv, sc.out_exp).to(DEV)
    q3 = torch.empty(3, M, 3 * D, dtype=torch.bfloat16, device=DEV)
    ops.split3(qkv, q3)
    qk = sc.qk_exp.to(DEV)
    ev = sc.out_exp[2 * D:]
    o2 = torch.full((2, D // 32, M, 32), float("nan"), dtype=torch.float16, device=DEV)
    o2b = torch.full((2, D // 32, M, 32), float("nan"), dtype=torch.float16, device=DEV)
    o3 = torch.full((3, D // 32, M, 32), float("nan"), dtype=torch.bfloat16, device=DEV)
    o23 = torch.full((3, D // 32, M, 32), float("nan"), dtype=torch.bfloat16, device=DEV)     # the new kernel writing three bf16 planes of the output itself
    op_checks._flush_caches()
    ops.vit_attention_f16x2(q2, o23, B, S, HEADS, qk, v_exp=ev.to(DEV).contiguous())
    op_checks._flush_caches()
    ops.vit_attention_f16x2(q2, o2, B, S, HEADS, qk)
    op_checks._flush_caches()
    ops.vit_attention_f16x2(q2, o2b, B, S, HEADS, qk)
    op_checks._flush_caches()
    ops.vit_attention(q3, o3, B, S, HEADS)
    torch.cuda.synchronize()
    assert torch.equal(o2.view(torch.int16), o2b.view(torch.int16)), "two launches differ"
    a = _kmaj2_rows(o2, ev)
    c = pk.kmajor_to_rows(o3.cpu()).double().sum(0)
    assert not torch.isnan(a).any() and not torch.isnan(c).any()
    a3 = pk.kmajor_to_rows(o23.cpu()).double().sum(0)
    assert not torch.isnan(a3).any()
    e2, e3, e23 = _errs(a, ref, mag), _errs(c, ref, mag), _errs(a3, ref, mag)
    print(f"attention B={B} {'dynamic-range' if wide else 'plain'}: fp16x2 elem {e2[0]:.3e} norm {e2[1]:.3e} (bf16 planes out: elem {e23[0]:.3e} norm {e23[1]:.3e}) "
          f"| bf16x3 elem {e3[0]:.3e} norm {e3[1]:.3e}")
    assert e2[0] <= 2 * e3[0] and e2[1] <= 2 * e3[1], (e2, e3)
    assert e23[0] <= 2 * e3[0] and e23[1] <= 2 * e3[1], (e23, e3)


@pytest.mark.parametrize("wide", [False, True], ids=["plain", "dynamic_range"])
@pytest.mark.parametrize("B", [8, 1])
def test_projection_matches_float64_within_twice_bf16x3(B, wide):
    w, x, h, qkv, bn1, sc = _case(B, wide)
    M = B * S
    att = _attn64(qkv, B)[0].float()                     # the projection's float32 input, the same for both routes
    rows = f64_ref.sample_rows(M)
    ref, mag = f64_ref.linear_ref(att, w["attn.proj.weight"], w["attn.proj.bias"], scale=w["ls1.gamma"], res=x, rows=rows)
    pw2 = pk.pack_conv_f16x2(w["attn.proj.weight"], w["attn.proj.bias"], w["ls1.gamma"], sc.v_bound).to(DEV)
    pw3 = pk.pack_conv_split3(w["attn.proj.weight"], w["attn.proj.bias"], scale=w["ls1.gamma"], kmajor=True).to(DEV)
    assert torch.equal(pw2.in_exp.cpu(), sc.out_exp[2 * D:].cpu())
    a2 = pk.rows_to_kmajor(_planes2_rows(att, pw2.in_exp)).to(DEV)
    a3 = pk.rows_to_kmajor(torch.stack(pk.split3(att))).to(DEV)
    xd = x.to(DEV)
    y2 = torch.full((M, D), float("nan"), device=DEV)
    y3 = torch.full((M, D), float("nan"), device=DEV)
    op_checks._flush_caches()
    ops.conv_f16x2(a2, pw2, y2, res=xd)
    op_checks._flush_caches()
    ops.conv_split3(a3, pw3, y3, res=xd)
    torch.cuda.synchronize()
    assert not torch.isnan(y2).any() and not torch.isnan(y3).any()
    e2, e3 = f64_ref.errors(y2[rows.to(DEV)], ref, mag), f64_ref.errors(y3[rows.to(DEV)], ref, mag)
    print(f"projection B={B} {'dynamic-range' if wide else 'plain'}: fp16x2 elem {e2[0]:.3e} norm {e2[1]:.3e} | bf16x3 elem {e3[0]:.3e} norm {e3[1]:.3e}")
    assert e2[0] <= 2 * e3[0] and e2[1] <= 2 * e3[1], (e2, e3)


@pytest.mark.parametrize("wide", [False, True], ids=["plain", "dynamic_range"])
@pytest.mark.parametrize("B", [8, 1])
def test_qkv_row_major_planes_match_float64_within_twice_bf16x3(B, wide):
    """LayerNorm planes -> qkv as two fp16 row-major planes of y / 2^out_exp (the new store form) against the same launch storing three bf16 planes"""
    w, x, h, qkv, bn1, sc = _case(B, wide)
    M = B * S
    rows = f64_ref.sample_rows(M)
    pw = pk.pack_conv_f16x2(w["attn.qkv.weight"], w["attn.qkv.bias"], None, bn1).to(DEV)
    h2 = pk.rows_to_kmajor(_planes2_rows(h, pw.in_exp)).to(DEV)
    hq = torch.ldexp(h2.cpu().double().sum(0).permute(1, 0, 2).reshape(M, D), pw.in_exp.cpu().double()[None, :])      # what the planes hold, exactly
    ref, mag = f64_ref.linear_ref(hq, w["attn.qkv.weight"], w["attn.qkv.bias"], rows=rows)
    oe = sc.out_exp.to(DEV)
    y2 = torch.full((2, M, 3 * D), float("nan"), dtype=torch.float16, device=DEV)
    y3 = torch.full((3, M, 3 * D), float("nan"), dtype=torch.bfloat16, device=DEV)
    op_checks._flush_caches()
    ops.conv_f16x2(h2, pw, y2, out_exp=oe)
    op_checks._flush_caches()
    ops.conv_f16x2(h2, pw, y3)
    torch.cuda.synchronize()
    assert not torch.isnan(y2).any() and not torch.isnan(y3).any()          # every element written, none overflowed its static scale
    assert float(y2[0].float().abs().max()) <= 2.0 ** 14 * (1 + 2.0 ** -10)
    a = torch.ldexp(y2.double().sum(0).cpu(), sc.out_exp.double()[None, :])[rows]
    c = y3.double().sum(0).cpu()[rows]
    e2, e3 = f64_ref.errors(a, ref, mag), f64_ref.errors(c, ref, mag)
    print(f"qkv planes B={B} {'dynamic-range' if wide else 'plain'}: fp16x2 elem {e2[0]:.3e} norm {e2[1]:.3e} | bf16x3 elem {e3[0]:.3e} norm {e3[1]:.3e}")
    assert e2[0] <= 2 * e3[0] and e2[1] <= 2 * e3[1], (e2, e3)


@pytest.mark.parametrize("planes3", [False, True], ids=["fp16x2_out", "bf16x3_out"])
@pytest.mark.parametrize("B", [1, 8])
def test_non_finite_inputs_come_out_non_finite(B, planes3):
    """both output forms; B = 8 puts the poisoned rows in the LAST image, whose last query block (13 queries) runs the key-split path"""
    w, x, h, qkv, bn1, sc = _case(B, False)
    qkv = qkv.clone()
    v = qkv.view(B, S, 3, HEADS, 64)
    b = B - 1
    v[b, 5, 0, 2, 7] = float("nan")                      # q of token 5, head 2
    v[b, 1030, 0, 3, 1] = float("nan")                   # q of a token of the 13-query tail block, head 3
    v[b, 900, 1, 4, 0] = float("inf")                    # k of token 900, head 4: every query of the head
    v[b, 1036, 2, 7, 33] = float("-inf")                 # v of the last token, head 7, channel 33: that channel of every query
    q2 = _planes2_rows(qkv, sc.out_exp).to(DEV)
    if planes3:
        o = torch.zeros((3, D // 32, B * S, 32), dtype=torch.bfloat16, device=DEV)
        ops.vit_attention_f16x2(q2, o, B, S, HEADS, sc.qk_exp.to(DEV), v_exp=sc.out_exp[2 * D:].to(DEV).contiguous())
    else:
        o = torch.zeros((2, D // 32, B * S, 32), dtype=torch.float16, device=DEV)
        ops.vit_attention_f16x2(q2, o, B, S, HEADS, sc.qk_exp.to(DEV))
    torch.cuda.synchronize()
    out = pk.kmajor_to_rows(o.cpu()).double().sum(0).view(B, S, HEADS, 64)
    assert not torch.isfinite(out[b, 5, 2]).any()
    assert not torch.isfinite(out[b, 1030, 3]).any()
    assert not torch.isfinite(out[b, :, 4]).any()
    assert not torch.isfinite(out[b, :, 7, 33]).any()
    assert torch.isfinite(out[b, :, 0]).all() and torch.isfinite(out[b, 6, 2]).all() and torch.isfinite(out[b, 1031, 3]).all()
    if B > 1:
        assert torch.isfinite(out[0]).all()              # other images are untouched


def test_short_and_ragged_sequences():
    """S below one key block, S a multiple of 32, a head count that is not a multiple of 8 (block order fallback), the key-split tail"""
    g = torch.Generator().manual_seed(5)
    for (B, s, heads) in ((1, 13, 2), (3, 64, 4), (2, 300, 6), (1, 33, 1), (1, 269, 8)):
        d = heads * 64
        qkv = torch.randn(B * s, 3 * d, generator=g).to(DEV)
        q, k, v = qkv.double().view(B, s, 3, heads, 64).permute(2, 0, 3, 1, 4)
        ref = (((q * 0.125) @ k.transpose(-2, -1)).softmax(-1) @ v).transpose(1, 2).reshape(B * s, d).cpu()
        exp = torch.full((3 * d,), -11, dtype=torch.int32)                      # |N(0, 1)| < 8 = 2^(14 - 11)
        q2 = _planes2_rows(qkv, exp).to(DEV)
        o2 = torch.full((2, d // 32, B * s, 32), float("nan"), dtype=torch.float16, device=DEV)
        ops.vit_attention_f16x2(q2, o2, B, s, heads, torch.full((heads,), -22, dtype=torch.int32, device=DEV))
        torch.cuda.synchronize()
        a = _kmaj2_rows(o2, exp[2 * d:])
        assert not torch.isnan(a).any(), (B, s, heads)
        err = float((a - ref).abs().max()) / max(1.0, float(ref.abs().max()))
        assert err < 3e-6, (B, s, heads, err)                  # the float32-grade bar of op_checks.vit_attention_split3_v2


@pytest.mark.parametrize("value", ["0", "1", "2"])
def test_engine_switch_values_against_the_oracle(value, monkeypatch):
    """PF_VIT_ATTN_F16X2 = 0 / 1 / 2 end to end (the configuration of smoke()): the crops branch takes the routes the value names, the coarse
    branch none of them, and the depth map stays within the headline-parity bar (2e-5 in depth units, tests/test_headline_parity_gpu.py) of the
    oracle for every value"""
    from oracle import pf_oracle
    from patchfusion_amd.config import make_config
    from patchfusion_amd.model import PatchFusion
    from patchfusion_amd.spec import patchfusion_spec, synthetic_state_dict
    monkeypatch.setenv("PF_VIT_ATTN_F16X2", value)
    cfg = make_config("vits", (112, 154), (448, 616), (2, 2))
    sd = synthetic_state_dict(patchfusion_spec(cfg), 0)
    img = torch.rand(1, 3, 448, 616, generator=torch.Generator().manual_seed(1234))
    m = PatchFusion(cfg, compute_dtype="fp32").eval()
    m.load_state_dict(sd, strict=True)
    m = m.to("cuda:0")
    lr = m.resizer(img)
    d, _ = m(mode="infer", image_lr=lr.cuda(), image_hr=img.cuda(), cai_mode="m1", process_num=4)
    fine = m._engine["fine"]
    assert fine.f16x2 and (fine.attn_f16x2, fine.proj_f16x2) == {"0": (False, False), "1": (True, False), "2": (True, True)}[value]
    assert not m._engine["coarse"].attn_f16x2
    ref = pf_oracle.Oracle(cfg, sd).infer(lr, img, "m1", 4)
    err = float((d.cpu() - ref).abs().max())
    print(f"PF_VIT_ATTN_F16X2={value}: max |depth - oracle| = {err:.3e}")
    assert err <= 2e-5, err
