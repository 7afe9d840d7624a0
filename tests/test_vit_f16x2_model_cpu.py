"""CPU model of the static scales of the fp16x2 ViT block linears (packing.pack_conv_f16x2 / layernorm_bound / gelu_linear_bound / bound_exponents):
the bounds are never exceeded (random rows, a single-spike LayerNorm row that reaches sqrt(D - 1), the large-dynamic-range weights of
tests/dynamic_range.py), every scaled operand fits fp16 with the headroom the rule promises, and the fp16x2 reconstruction of a float32 operand is
within 2^-22 of its channel bound."""
import math

import torch

from patchfusion_amd import packing as pk
from patchfusion_amd.config import make_config
from patchfusion_amd.spec import patchfusion_spec, synthetic_state_dict
from tests.dynamic_range import widen_dynamic_range


def _ln(x, g, b, eps=1e-6):
    return torch.nn.functional.layer_norm(x, (x.shape[-1],), g.to(x.dtype), b.to(x.dtype), eps)


def _recon(v, e):
    """float32 operand -> its fp16x2 planes under exponents e -> float64 value"""
    h, l = pk.split_f16x2(torch.ldexp(v.double(), -e.double()).float())
    return torch.ldexp(h.double() + l.double(), e.double())


def test_bound_exponents_rule():
    b = torch.tensor([0.0, 1.0, 1.5, 2.0 ** 14, 2.0 ** 14 + 1, 3e-7, 7e4], dtype=torch.float64)
    e = pk.bound_exponents(b)
    assert e.dtype == torch.int32 and int(e[0]) == 0
    for bi, ei in zip(b[1:].tolist(), e[1:].tolist()):
        assert bi / 2.0 ** ei <= 2.0 ** 14 < bi / 2.0 ** (ei - 1)     # the smallest e with bound / 2^e <= 2^14


def test_layernorm_bound_holds_and_is_reached_by_a_spike():
    D = 1024
    g = torch.Generator().manual_seed(0)
    gamma, beta = torch.randn(D, generator=g), torch.randn(D, generator=g) * 0.1
    bound = pk.layernorm_bound(gamma, beta)
    rows = torch.cat([torch.randn(256, D, generator=g, dtype=torch.float64) * 10 ** torch.randn(256, 1, generator=g, dtype=torch.float64),
                      torch.randn(64, D, generator=g, dtype=torch.float64) ** 7])
    y = _ln(rows, gamma.double(), beta.double())
    assert (y.abs() <= bound[None, :] * (1 + 1e-12)).all()
    spike = torch.zeros(D, D, dtype=torch.float64)
    spike.diagonal().fill_(1e3)                                  # row k: one spike in channel k -> x_hat_k = sqrt(D - 1) (up to eps)
    xh = _ln(spike, torch.ones(D), torch.zeros(D))
    assert abs(float(xh.diagonal().min()) / math.sqrt(D - 1) - 1) < 1e-9
    ys = _ln(spike, gamma.double(), beta.double()).diagonal()
    assert (ys.abs() <= bound * (1 + 1e-12)).all()
    assert float((ys.abs() / bound).max()) > 0.999
    # float32 LayerNorm of the spike rows, scaled: inside 2^14 up to the float32 rounding the headroom bit is there for, far from fp16's 65504
    e = pk.bound_exponents(bound)
    t = torch.ldexp(_ln(spike.float(), gamma, beta).double(), -e.double()[None, :])
    assert float(t.abs().max()) <= 2.0 ** 14 * (1 + 2 ** -20)


def test_gelu_bound_holds():
    D, H = 256, 1024
    g = torch.Generator().manual_seed(1)
    gamma, beta = torch.randn(D, generator=g), torch.randn(D, generator=g) * 0.1
    w1, b1 = torch.randn(H, D, generator=g) / D ** 0.5, torch.randn(H, generator=g)
    lb = pk.layernorm_bound(gamma, beta)
    gb = pk.gelu_linear_bound(w1, b1, lb)
    assert (gb >= 0.17).all()
    x = torch.cat([torch.randn(512, D, generator=g, dtype=torch.float64), torch.eye(D, dtype=torch.float64) * 50])
    z = _ln(x, gamma.double(), beta.double()) @ w1.double().t() + b1.double()
    assert (torch.nn.functional.gelu(z).abs() <= gb[None, :]).all()
    # the row that aligns every input with the signs of W1[n] reaches the linear bound (before GELU) exactly
    n = 3
    yk = torch.sign(w1[n].double()) * lb
    assert abs(float(yk @ w1[n].double() + abs(float(b1[n]))) - float(gb[n])) <= 1e-9 * float(gb[n])


def test_reconstruction_within_2m22_of_the_channel_bound():
    g = torch.Generator().manual_seed(2)
    C = 512
    bound = 10 ** (torch.rand(C, generator=g, dtype=torch.float64) * 12 - 6)            # channel bounds over twelve decades
    e = pk.bound_exponents(bound)
    mag = 10 ** (-torch.rand(2048, C, generator=g, dtype=torch.float64) * 8)            # values 0 .. 8 decades below their bound
    v = (torch.sign(torch.randn(2048, C, generator=g, dtype=torch.float64)) * mag * bound[None, :]).float()
    v[0] = bound.float() * (1 - 2 ** -24)                                               # the bound itself (float32 below it)
    r = _recon(v, e)
    assert ((r - v.double()).abs() <= 2.0 ** -22 * bound[None, :]).all()
    # relative precision holds down to 2^17 below the bound (where the l plane reaches fp16's subnormals)
    near = v.double().abs() >= bound[None, :] * 2.0 ** -17
    rel = ((r - v.double()).abs() / v.double().abs().clamp_min(1e-300))[near]
    assert float(rel.max()) <= 2.0 ** -21


def test_weight_planes_reconstruct_and_fit_fp16():
    g = torch.Generator().manual_seed(3)
    K, N = 256, 96
    w = torch.randn(N, K, generator=g) * 10 ** (torch.rand(N, 1, generator=g) * 6 - 3)
    w[5] = 0                                                                            # a zero row: f_n = 0
    bound = 10 ** (torch.rand(K, generator=g, dtype=torch.float64) * 6 - 3)
    pw = pk.pack_conv_f16x2(w, torch.randn(N, generator=g), None, bound)
    assert pw.w.dtype == torch.float16 and tuple(pw.w.shape) == (2, K // 32, 96, 32)
    assert pw.col_exp.dtype == pw.in_exp.dtype == torch.int32 and int(pw.col_exp[5]) == 0
    planes = pk.kmajor_to_rows(pw.w).double()
    assert float(planes.sum(0).abs().max()) <= 2.0 ** 15
    rec = torch.ldexp(planes.sum(0), pw.col_exp.double()[:, None] - pw.in_exp.double()[None, :])[:N]
    # error per weight <= 2^-22 of the largest scaled weight of its row
    rowmax = (w.double().abs() * torch.ldexp(torch.ones(K, dtype=torch.float64), pw.in_exp.double())[None, :]).amax(1, keepdim=True)
    err = (rec - w.double()).abs() * torch.ldexp(torch.ones(K, dtype=torch.float64), pw.in_exp.double())[None, :]
    assert (err <= 2.0 ** -22 * rowmax + 1e-300).all()


def test_dynamic_range_weights_stay_inside_their_bounds():
    """the ViT blocks of the large-dynamic-range state dict: LayerNorm outputs and GELU(fc1) of random token rows never exceed the static bounds,
    and every scaled operand fits fp16"""
    cfg = make_config("vits", (112, 154), (448, 616), (2, 2))
    sd = widen_dynamic_range(synthetic_state_dict(patchfusion_spec(cfg), 0))
    g = torch.Generator().manual_seed(4)
    pre = "coarse_branch.core.core.pretrained.blocks."
    for i in (0, 5, 11):
        b = f"{pre}{i}."
        n2 = (sd[b + "norm2.weight"], sd[b + "norm2.bias"])
        D = n2[0].numel()
        x = torch.randn(300, D, generator=g) * 10 ** (torch.rand(300, 1, generator=g) * 4 - 2) + torch.randn(D, generator=g) * 3
        x[:D] += torch.eye(D)[:300] * 1e4                                        # spikes
        lb = pk.layernorm_bound(*n2)
        y = _ln(x, *n2)
        assert (y.double().abs() <= lb[None, :] * (1 + 2 ** -20)).all()
        w1, b1 = sd[b + "mlp.fc1.weight"], sd[b + "mlp.fc1.bias"]
        gb = pk.gelu_linear_bound(w1, b1, lb)
        z = torch.nn.functional.gelu(y.double() @ w1.double().t() + b1.double())
        assert (z.abs() <= gb[None, :]).all()
        for v, bound in ((y, lb), (z.float(), gb)):
            e = pk.bound_exponents(bound)
            t = torch.ldexp(v.double(), -e.double()[None, :])
            assert float(t.abs().max()) <= 2.0 ** 14 * (1 + 2 ** -20)
            assert ((_recon(v, e) - v.double()).abs() <= 2.0 ** -22 * bound[None, :]).all()
