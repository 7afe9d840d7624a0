"""pytest -m gpu: the fp16x2 ViT block linears (csrc/gemm_split3.hip pf_gemm_f16x2, csrc/vit.hip pf_layernorm_f16x2) against float64, next to the
bf16x3 route (pf_layernorm_split3 + pf_gemm_split3) on the same float32 inputs.

qkv 1024->3072 (LayerNorm in, three bf16 planes out), fc1 1024->4096 (LayerNorm in, GELU, fp16x2 planes out for fc2) and fc2 4096->1024 (fp16x2
planes of GELU values in, bias -> LayerScale -> residual, float32 out) at the pass's token counts M = 8296 and 1037.  The error of the fp16x2 route
(max |y - ref| / max |ref|) must stay within 4x the bf16x3 route's, every element of the NaN-filled outputs must be written, and every checked
launch starts from cold caches (op_checks._flush_caches).  The projection keeps the bf16x3 route and is covered by tests/op_checks.py."""
import math

import pytest
import torch

from patchfusion_amd import packing as pk
from patchfusion_amd.hip_ops import ops
from tests import op_checks

pytestmark = pytest.mark.gpu
DEV = "cuda"
D = 1024


def _ln_case(M, seed):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(M, D, generator=g) * (0.5 + torch.rand(D, generator=g)) + torch.randn(D, generator=g)).float()
    gamma = (torch.randn(D, generator=g) * 0.5).float()
    beta = (torch.randn(D, generator=g) * 0.2).float()
    return x, gamma, beta


def _ln64(x, gamma, beta):
    return torch.nn.functional.layer_norm(x.double(), (x.shape[1],), gamma.double(), beta.double(), 1e-6)


def _f16x2_rows(y2, exp):
    """two fp16 planes [2, N/32, M, 32] of y / 2^exp -> float64 [M, N]"""
    return torch.ldexp(pk.kmajor_to_rows(y2.cpu()).double().sum(0), exp.cpu().double()[None, :])


def _err(y, ref):
    return float((y - ref).abs().max() / ref.abs().max())


@pytest.mark.parametrize("M", [8 * 1037, 1037])
@pytest.mark.parametrize("name", ["qkv", "fc1"])
def test_layernorm_linear_matches_float64(name, M):
    N = 3 * D if name == "qkv" else 4 * D
    x, gamma, beta = _ln_case(M, 1 + N)
    g = torch.Generator().manual_seed(7 + N)
    w = (torch.randn(N, D, generator=g) / D ** 0.5).float()
    b = torch.randn(N, generator=g).float()
    act = "gelu" if name == "fc1" else None
    z = _ln64(x, gamma, beta) @ w.double().t() + b.double()
    ref = torch.nn.functional.gelu(z) if act else z
    bound = pk.layernorm_bound(gamma, beta)
    pw = pk.pack_conv_f16x2(w, b, None, bound).to(DEV)
    pw3 = pk.pack_conv_split3(w, b, kmajor=True).to(DEV)
    xd, gd, bd = x.to(DEV), gamma.to(DEV), beta.to(DEV)
    h2 = torch.empty(2, D // 32, M, 32, dtype=torch.float16, device=DEV)
    h3 = torch.empty(3, D // 32, M, 32, dtype=torch.bfloat16, device=DEV)
    if name == "fc1":                                    # fp16x2 planes for fc2, with fc2's input exponents
        out_exp = pk.bound_exponents(pk.gelu_linear_bound(w, b, bound)).to(DEV)
        y2 = torch.full((2, N // 32, M, 32), float("nan"), dtype=torch.float16, device=DEV)
        y3 = torch.full((3, N // 32, M, 32), float("nan"), dtype=torch.bfloat16, device=DEV)
    else:                                                # three bf16 row-major planes for the attention
        out_exp = None
        y2 = torch.full((3, M, N), float("nan"), dtype=torch.bfloat16, device=DEV)
        y3 = torch.full((3, M, N), float("nan"), dtype=torch.bfloat16, device=DEV)
    op_checks._flush_caches()
    ops.layernorm_f16x2(xd, h2, gd, bd, 1e-6, pw.in_exp)
    op_checks._flush_caches()
    ops.conv_f16x2(h2, pw, y2, act=act, out_exp=out_exp)
    op_checks._flush_caches()
    ops.layernorm_split3(xd, h3, gd, bd, 1e-6)
    op_checks._flush_caches()
    ops.conv_split3(h3, pw3, y3, act=act)
    torch.cuda.synchronize()
    if name == "fc1":
        a = _f16x2_rows(y2, out_exp)
        c = pk.kmajor_to_rows(y3.cpu()).double().sum(0)
    else:
        a, c = y2.cpu().double().sum(0), y3.cpu().double().sum(0)
    assert not torch.isnan(a).any() and not torch.isnan(c).any()
    e16, e3 = _err(a, ref), _err(c, ref)
    print(f"{name} M={M}: fp16x2 {e16:.2e}  bf16x3 {e3:.2e}")
    assert e16 <= 4 * e3, (e16, e3)
    assert e16 < 1e-6


@pytest.mark.parametrize("M", [8 * 1037, 1037])
def test_fc2_matches_float64(M):
    K, N = 4 * D, D
    g = torch.Generator().manual_seed(11)
    w1 = (torch.randn(K, D, generator=g) / D ** 0.5).float()
    b1 = torch.randn(K, generator=g).float()
    bound = pk.gelu_linear_bound(w1, b1, pk.layernorm_bound(torch.ones(D), torch.zeros(D)))
    mid = torch.nn.functional.gelu(torch.randn(M, K, generator=g, dtype=torch.float64) * 2).float()
    w = (torch.randn(N, K, generator=g) / K ** 0.5).float()
    b = torch.randn(N, generator=g).float()
    ls = (0.5 + torch.rand(N, generator=g)).float()
    res = torch.randn(M, N, generator=g).float()
    ref = (mid.double() @ w.double().t() + b.double()) * ls.double() + res.double()
    pw = pk.pack_conv_f16x2(w, b, ls, bound).to(DEV)
    pw3 = pk.pack_conv_split3(w, b, scale=ls, kmajor=True).to(DEV)
    m2 = pk.rows_to_kmajor(torch.stack(pk.split_f16x2(torch.ldexp(mid.double(), -pw.in_exp.cpu().double()[None, :]).float()))).to(DEV)
    m3 = pk.rows_to_kmajor(torch.stack(pk.split3(mid))).to(DEV)
    resd = res.to(DEV)
    y2 = torch.full((M, N), float("nan"), device=DEV)
    y3 = torch.full((M, N), float("nan"), device=DEV)
    op_checks._flush_caches()
    ops.conv_f16x2(m2, pw, y2, res=resd)
    op_checks._flush_caches()
    ops.conv_split3(m3, pw3, y3, res=resd)
    torch.cuda.synchronize()
    a, c = y2.cpu().double(), y3.cpu().double()
    assert not torch.isnan(a).any() and not torch.isnan(c).any()
    e16, e3 = _err(a, ref), _err(c, ref)
    print(f"fc2 M={M}: fp16x2 {e16:.2e}  bf16x3 {e3:.2e}")
    assert e16 <= 4 * e3, (e16, e3)
    assert e16 < 4e-6


def test_few_tiles_and_ragged_rows():
    """fewer 192 x 192 tiles than XCDs (the launch still walks with 8 blocks) and a token count that is not a multiple of 192"""
    M, N = 77, 256
    x, gamma, beta = _ln_case(M, 3)
    g = torch.Generator().manual_seed(5)
    w = (torch.randn(N, D, generator=g) / D ** 0.5).float()
    b = torch.randn(N, generator=g).float()
    ref = _ln64(x, gamma, beta) @ w.double().t() + b.double()
    pw = pk.pack_conv_f16x2(w, b, None, pk.layernorm_bound(gamma, beta)).to(DEV)
    h2 = torch.empty(2, D // 32, M, 32, dtype=torch.float16, device=DEV)
    y = torch.full((M, N + 4), float("nan"), device=DEV)
    ops.layernorm_f16x2(x.to(DEV), h2, gamma.to(DEV), beta.to(DEV), 1e-6, pw.in_exp)
    ops.conv_f16x2(h2, pw, y[:, :N])
    torch.cuda.synchronize()
    a = y.cpu().double()
    assert torch.isnan(a[:, N:]).all()                   # nothing beyond the N columns is written
    assert not torch.isnan(a[:, :N]).any()
    assert _err(a[:, :N], ref) < 1e-6
    assert math.isfinite(_err(a[:, :N], ref))
