"""tests/head_bwd_ref.py (the backward formulas of csrc/head_bwd.hip without autograd) against torch.autograd through oracle/pf_oracle.py,
float64: every tensor within 1e-10 of the autograd gradient, relative to that tensor's largest entry."""
import pytest
import torch

from oracle import pf_oracle
from tests import head_bwd_ref as R

F64 = torch.float64
TOL = 1e-10


def rel_err(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


@pytest.mark.parametrize("at", ["inv", "exp"])
@pytest.mark.parametrize("ak", ["mean", "sum"])
@pytest.mark.parametrize("with_rel", [False, True])
def test_whole_head_restatement_matches_autograd(at, ak, with_rel):
    sd, bcfg, inp, target = R.probe_head(at, ak, with_rel)
    loss, depth, pg, ig = R.oracle_head_grads(sd, bcfg, inp, target)
    sd64 = {k: v.to(F64) if v.is_floating_point() else v for k, v in sd.items()}
    d = lambda t: None if t is None else t.to(F64)
    got_depth, ctx = R.head_forward(sd64, "", d(inp["x0"]), [d(t) for t in inp["x_blocks"]], d(inp["last"]), d(inp["rel"]), bcfg)
    assert rel_err(got_depth, depth) <= TOL
    valid = int(((target > bcfg["min_depth"]) & (target < bcfg["max_depth"])).sum())
    assert 0.7 * target.numel() < valid < 0.9 * target.numel()
    d_depth = R.silog_bwd(got_depth, target.to(F64), bcfg["min_depth"], bcfg["max_depth"])
    grads, inputs = R.head_backward(sd64, "", ctx, bcfg, d_depth)
    assert len(pg) == 44 and set(grads) == set(pg)          # 22 layers: 2 seed MLPs, 4 projectors, 4 attractors (two layers each), mlp.0, mlp.2
    for k in pg:
        assert float(pg[k].abs().max()) > 0 and grads[k].shape == pg[k].shape, k
        assert rel_err(grads[k], pg[k]) <= TOL, k
    flat = lambda g: [g["x0"], *g["x_blocks"], g["last"]] + ([g["rel"]] if "rel" in g else [])
    assert ("rel" in inputs) == with_rel and len(flat(inputs)) == len(flat(ig)) == 6 + with_rel
    for a, b in zip(flat(inputs), flat(ig)):
        assert float(b.abs().max()) > 0 and rel_err(a, b) <= TOL


@pytest.mark.parametrize("src,dst", [((2, 3), (3, 5)), ((1, 1), (4, 4)), ((5, 7), (5, 7)), ((17, 25), (33, 49))])
def test_resize_adjoint_identity_and_forward(src, dst):
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, *src, 3, generator=g, dtype=F64)
    gy = torch.randn(2, *dst, 3, generator=g, dtype=F64)
    up = R.resize_fwd(x, *dst)
    assert rel_err(up, pf_oracle.up(x.permute(0, 3, 1, 2), dst).permute(0, 2, 3, 1)) <= 1e-14
    lhs, rhs = float((up * gy).sum()), float((x * R.resize_bwd(gy, *src)).sum())
    assert abs(lhs - rhs) <= 1e-12 * max(1.0, abs(lhs))
    if src == dst:
        assert torch.equal(R.resize_bwd(gy, *src), gy)
    if src == (1, 1):
        assert torch.allclose(R.resize_bwd(gy, 1, 1)[:, 0, 0], gy.sum((1, 2)), rtol=1e-14, atol=0)


def _silog_autograd(pred, target, lo, hi):
    p = pred.clone().requires_grad_(True)
    loss = pf_oracle.silog_loss(p, target, lo, hi)
    loss.sum().backward()
    return p.grad


def test_silog_backward_partial_mask_and_single_valid_pixel():
    g = torch.Generator().manual_seed(5)
    pred = torch.rand(2, 1, 9, 13, generator=g, dtype=F64) * 60 + 1
    target = torch.rand(2, 1, 9, 13, generator=g, dtype=F64) * 100 - 5
    want = _silog_autograd(pred, target, 1e-3, 80.0)
    assert 0 < int((want != 0).sum()) < want.numel()
    assert rel_err(R.silog_bwd(pred, target, 1e-3, 80.0), want) <= TOL
    assert rel_err(R.silog_bwd(pred, target, 1e-3, 80.0, d_loss=0.25), 0.25 * want) <= TOL
    one = torch.full_like(target, -1.0)
    one[1, 0, 4, 6] = 10.0
    assert not _silog_autograd(pred, one, 1e-3, 80.0).any() and not R.silog_bwd(pred, one, 1e-3, 80.0).any()
    full = target.clamp(1.0, 70.0)
    assert rel_err(R.silog_bwd(pred, full, 1e-3, 80.0), _silog_autograd(pred, full, 1e-3, 80.0)) <= TOL


def test_logbinom_backward_where_both_clamps_bind():
    pt, cen, gd = logbinom_case(F64)
    p = pt.clone().requires_grad_(True)
    c = cen.clone().requires_grad_(True)
    R.logbinom_fwd(p, c, 0.0212, 50.0).backward(gd)
    prob = (pt[..., 0] + 1e-4) / (pt[..., 0] + pt[..., 1] + 2e-4)
    assert int((prob < 1e-4).sum()) > 0 and int((1 - prob < 1e-4).sum()) > 0 and int(((prob > 0.1) & (prob < 0.9)).sum()) > 0
    d_pt, d_cup = R.logbinom_bwd(pt, cen, gd, 0.0212, 50.0)
    assert rel_err(d_pt, p.grad) <= TOL and rel_err(R.resize_bwd(d_cup, 5, 7), c.grad) <= TOL


def logbinom_case(dtype):
    """pt [2,9,13,4] with rows whose probability falls below 1e-4 (the clamp of x binds) and above 1 - 1e-4 (the clamp of 1 - x binds);
    centres at (5, 7); an upstream gradient"""
    g = torch.Generator().manual_seed(7)
    pt = torch.rand(2, 9, 13, 4, generator=g, dtype=F64) * 2 + 0.05
    pt[:, 0, :, 0], pt[:, 0, :, 1] = 1e-6, 30.0           # prob ~ 3e-6
    pt[:, 1, :, 0], pt[:, 1, :, 1] = 30.0, 1e-6           # 1 - prob ~ 3e-6
    pt[..., 2] *= 0.1                                     # temperatures around 4 rather than 25: the softmax is not flat
    cen = torch.rand(2, 5, 7, 64, generator=g, dtype=F64).cumsum(-1)
    gd = torch.randn(2, 9, 13, generator=g, dtype=F64)
    return pt.to(dtype), cen.to(dtype), gd.to(dtype)


@pytest.mark.parametrize("at", ["inv", "exp"])
@pytest.mark.parametrize("ak", ["mean", "sum"])
@pytest.mark.parametrize("n_attr", [1, 16])
def test_attractor_backward(at, ak, n_attr):
    A, bp, gb = attractor_case(n_attr, F64)
    a = A.clone().requires_grad_(True)
    b = bp.clone().requires_grad_(True)
    out = R.attractor_fwd(a, b, at, ak)
    ref, _ = pf_oracle.attractor_unnormed.__globals__["_attractor_delta"], None
    want = pf_oracle.up(bp.permute(0, 3, 1, 2), (5, 7)) + ref(A.permute(0, 3, 1, 2), pf_oracle.up(bp.permute(0, 3, 1, 2), (5, 7)),
                                                              dict(attractor_type=at, attractor_kind=ak))
    assert rel_err(out.detach(), want.permute(0, 2, 3, 1)) <= 1e-13
    out.backward(gb)
    dA, d_bc = R.attractor_bwd(A, bp, gb, at, ak)
    assert rel_err(dA, a.grad) <= TOL and rel_err(R.resize_bwd(d_bc, 3, 5), b.grad) <= TOL


def attractor_case(n_attr, dtype):
    """A [2,5,7,n_attr] and low-resolution centres [2,3,5,64] close enough that 300 dx^2 passes through 1 (f' changes sign)"""
    g = torch.Generator().manual_seed(11 + n_attr)
    A = torch.rand(2, 5, 7, n_attr, generator=g, dtype=F64) * 0.5
    bp = torch.rand(2, 3, 5, 64, generator=g, dtype=F64) * 0.5
    gb = torch.randn(2, 5, 7, 64, generator=g, dtype=F64)
    return A.to(dtype), bp.to(dtype), gb.to(dtype)


@pytest.mark.parametrize("act", ["relu", "softplus", "gelu"])
def test_activation_derivatives(act):
    import torch.nn.functional as F
    z = torch.linspace(-6, 6, 241, dtype=F64).requires_grad_(True)
    y = {"relu": torch.relu, "softplus": F.softplus, "gelu": F.gelu}[act](z)
    y.sum().backward()
    ref = z.detach() if act == "gelu" else y.detach()
    assert rel_err(R.act_bwd(torch.ones_like(ref), ref, act), z.grad) <= TOL


def test_weight_gradient_of_a_1x1_layer():
    g = torch.Generator().manual_seed(13)
    x = torch.randn(2, 3, 5, 12, generator=g, dtype=F64)
    w = torch.randn(7, 12, 1, 1, generator=g, dtype=F64, requires_grad=True)
    b = torch.randn(7, generator=g, dtype=F64, requires_grad=True)
    gy = torch.randn(2, 3, 5, 7, generator=g, dtype=F64)
    torch.nn.functional.conv2d(x.permute(0, 3, 1, 2), w, b).backward(gy.permute(0, 3, 1, 2))
    dw, db = R.wgrad(gy, x)
    assert rel_err(dw, w.grad.flatten(1)) <= 1e-13 and rel_err(db, b.grad) <= 1e-13
