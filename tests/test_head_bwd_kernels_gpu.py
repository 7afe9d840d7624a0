"""The backward kernels of csrc/head_bwd.hip, one by one, on the GPU.

Truth: the formulas of tests/head_bwd_ref.py in float64 on the CPU (held against float64 autograd in tests/test_head_bwd_ref_cpu.py).
Comparator: torch's own float32 kernels on the same device: autograd through the oracle's float32 lines (pf_oracle.up = F.interpolate,
pf_oracle._attractor_delta, pf_oracle.silog_loss; the log-binomial lines restated in head_bwd_ref.logbinom_fwd_up), torch.matmul for the
weight gradient.
Bar of a gradient tensor g:  max |g - g64| / max |g64|  <=  2 x (the comparator's same quantity) + f64_ref.BASE_FLOOR -- the factor 2 is the
margin every grade test of this project gives over its comparator (a different, equally valid summation order).  The weight-gradient kernel
is held element by element instead: |dW - ref| / mag with mag = sum_p |dy| |x| against torch.matmul's on the same operands (the idiom of
f64_ref.float32_grade).  Every test also runs its kernel twice and asks for identical bits (no float atomics, fixed summation orders)."""
import pytest
import torch
import torch.nn.functional as F

from oracle import pf_oracle
from tests import head_bwd_ref as R
from tests.f64_ref import BASE_FLOOR, TINY
from tests.test_head_bwd_ref_cpu import attractor_case, logbinom_case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F64 = torch.float64


@pytest.fixture(scope="module")
def ops():
    from patchfusion_amd.hip_ops import ops
    return ops


def normwise(g, truth):
    g = g.detach().cpu().to(F64)
    if not torch.isfinite(g).all():
        return float("inf")
    return float((g - truth).abs().max() / max(float(truth.abs().max()), TINY))


def hold(name, got, truth, comp):
    e, base = normwise(got, truth), normwise(comp, truth)
    print(f"{name}: hip {e:.3e} comparator {base:.3e}")
    assert e <= 2 * base + BASE_FLOOR, (name, e, base)


def nan_like(shape):
    return torch.full(shape, float("nan"), device=DEV)


# ---------------- weight gradient ----------------
WGRAD = [(32, 256, 0, 0), (256, 64, 0, 0), (128, 128, 0, 0), (128, 1, 0, 0), (160, 80, 168, 0), (80, 4, 0, 8)]     # K, N, x_ld, dy_ld (0: dense)


@pytest.mark.parametrize("K,N,x_ld,dy_ld", WGRAD)
@pytest.mark.parametrize("P,rows", [(5, 0), (5, 2), (850, 0), (850, 288)])
def test_wgrad_elementwise_against_matmul(ops, K, N, x_ld, dy_ld, P, rows):
    """850 = 2 x 17 x 25 pixels; rows_per_block 288 -> partials of 288, 288 and a ragged 274 (not a multiple of the 32-pixel step), 2 -> 2, 2, 1;
    0 = the default (one or two partials here)"""
    g = torch.Generator().manual_seed(K * 1000 + N + P)
    shape = (2, 17, 25) if P == 850 else (1, 1, 5)
    xb = torch.randn(*shape, x_ld or K, generator=g).to(DEV)
    dyb = (torch.randn(*shape, dy_ld or N, generator=g) * torch.rand(*shape, 1, generator=g) * 3).to(DEV)
    x, dy = xb[..., :K], dyb[..., :N]
    if rows:
        assert -(-P // rows) >= 3 and P % rows
    dw, db = ops.conv1x1_wgrad(dy, x, nan_like((N, K)), nan_like((N,)), rows_per_block=rows)
    dw2, db2 = ops.conv1x1_wgrad(dy, x, nan_like((N, K)), nan_like((N,)), rows_per_block=rows)
    assert torch.equal(dw, dw2) and torch.equal(db, db2)
    d2, x2 = dy.reshape(-1, N), x.reshape(-1, K)
    d64, x64 = d2.cpu().to(F64), x2.cpu().to(F64)
    ref, mag = d64.t() @ x64, d64.abs().t() @ x64.abs()
    elem = lambda y, r, m: float(((y.cpu().to(F64) - r).abs() / (m + TINY)).max()) if torch.isfinite(y).all() else float("inf")
    e, base = elem(dw, ref, mag), elem(torch.matmul(d2.t(), x2), ref, mag)
    eb, baseb = elem(db, d64.sum(0), d64.abs().sum(0)), elem(d2.sum(0), d64.sum(0), d64.abs().sum(0))
    print(f"wgrad K={K} N={N} P={P} rows={rows}: dW hip {e:.3e} matmul {base:.3e}; db hip {eb:.3e} torch.sum {baseb:.3e}")
    assert e <= 2 * base + BASE_FLOOR and eb <= 2 * baseb + BASE_FLOOR
    assert not torch.isnan(xb).any() and not torch.isnan(dyb).any()


def test_wgrad_without_bias_and_with_a_short_workspace(ops):
    from patchfusion_amd._lib import PfError
    x, dy = torch.randn(1, 1, 40, 16, device=DEV), torch.randn(1, 1, 40, 8, device=DEV)
    dw, _ = ops.conv1x1_wgrad(dy, x, nan_like((8, 16)))
    assert torch.allclose(dw, dy.reshape(-1, 8).t() @ x.reshape(-1, 16), rtol=1e-5, atol=1e-5)
    with pytest.raises(PfError):
        ops.conv1x1_wgrad(dy, x, nan_like((8, 16)), rows_per_block=-1)


# ---------------- resize adjoint ----------------
@pytest.mark.parametrize("src,dst", [((2, 3), (3, 5)), ((1, 1), (4, 4)), ((5, 7), (5, 7)), ((17, 25), (33, 49))])
@pytest.mark.parametrize("accumulate", [False, True])
def test_resize_adjoint(ops, src, dst, accumulate):
    g = torch.Generator().manual_seed(17)
    gy = torch.randn(2, *dst, 8, generator=g).to(DEV)[..., :5]                    # an odd channel count in a wider buffer
    init = torch.randn(2, *src, 5, generator=g).to(DEV)
    dx = ops.resize_bwd(gy, init.clone() if accumulate else nan_like((2, *src, 5)), accumulate=accumulate)
    dx2 = ops.resize_bwd(gy, init.clone() if accumulate else nan_like((2, *src, 5)), accumulate=accumulate)
    assert torch.equal(dx, dx2)
    x = torch.zeros(2, 5, *src, device=DEV, requires_grad=True)
    pf_oracle.up(x, dst).backward(gy.permute(0, 3, 1, 2))
    comp = x.grad.permute(0, 2, 3, 1)
    truth = R.resize_bwd(gy.cpu().to(F64), *src)
    if accumulate:
        comp, truth = init + comp, init.cpu().to(F64) + truth
    hold(f"resize_bwd {src}->{dst} acc={accumulate}", dx, truth, comp)
    if src == dst and not accumulate:
        assert torch.equal(dx, gy)                                                # equal sizes: the identity, exactly
    # the adjoint identity <up(x), g> = <x, up^T(g)> on the kernel's own output
    if not accumulate:
        xr = torch.randn(2, *src, 5, generator=g).to(DEV)
        lhs = float((pf_oracle.up(xr.permute(0, 3, 1, 2), dst).permute(0, 2, 3, 1).double() * gy.double()).sum())
        rhs = float((xr.double() * dx.double()).sum())
        assert abs(lhs - rhs) <= 1e-5 * float((xr.abs().double() * R.resize_bwd(gy.abs().cpu().to(F64), *src).to(DEV)).sum())


# ---------------- attractor ----------------
@pytest.mark.parametrize("at", ["inv", "exp"])
@pytest.mark.parametrize("ak", ["mean", "sum"])
@pytest.mark.parametrize("n_attr", [1, 16])
def test_attractor_backward(ops, at, ak, n_attr):
    A, bp, gb = (t.to(DEV) for t in attractor_case(n_attr, torch.float32))
    run = lambda: ops.attractor_bwd(A, n_attr, bp, gb, nan_like((2, 5, 7, 24))[..., :n_attr], nan_like((2, 5, 7, 64)), attractor_type=at, kind=ak)
    (dA, d_bc), (dA2, d_bc2) = run(), run()
    assert torch.equal(dA, dA2) and torch.equal(d_bc, d_bc2)
    tA, t_bc = R.attractor_bwd(A.cpu().to(F64), bp.cpu().to(F64), gb.cpu().to(F64), at, ak)
    # comparator: the oracle's own float32 lines (attractor_unnormed: up = F.interpolate, _attractor_delta), NCHW, on this device
    bcfg = dict(attractor_type=at, attractor_kind=ak)
    nchw = lambda t: t.permute(0, 3, 1, 2).contiguous()
    a = nchw(A).requires_grad_(True)
    b = nchw(bp).requires_grad_(True)
    c = pf_oracle.up(b, (5, 7))
    c.retain_grad()                                                               # the gradient at the attractor's grid, like d_b_c
    (c + pf_oracle._attractor_delta(a, c, bcfg)).backward(nchw(gb))
    hold(f"attractor_bwd dA {at} {ak} n={n_attr}", dA, tA, a.grad.permute(0, 2, 3, 1))
    hold(f"attractor_bwd d_b_c {at} {ak} n={n_attr}", d_bc, t_bc, c.grad.permute(0, 2, 3, 1))
    # and the gradient of the low-resolution centres: the resize adjoint of d_b_c
    d_bp = ops.resize_bwd(d_bc, nan_like((2, 3, 5, 64)))
    hold(f"attractor_bwd d_b_prev {at} {ak} n={n_attr}", d_bp, R.resize_bwd(t_bc, 3, 5), b.grad.permute(0, 2, 3, 1))


# ---------------- log-binomial expectation ----------------
def test_logbinom_backward_with_both_clamps_binding(ops):
    pt, cen, gd = (t.to(DEV) for t in logbinom_case(torch.float32))
    ptb = torch.zeros(2, 9, 13, 8, device=DEV)
    ptb[..., :4] = pt
    run = lambda: ops.logbinom_depth_bwd(ptb[..., :4], cen, gd, nan_like((2, 9, 13, 8))[..., :4], nan_like((2, 9, 13, 64)), 0.0212, 50.0)
    (d_pt, d_cup), (d_pt2, d_cup2) = run(), run()
    assert torch.equal(d_pt, d_pt2) and torch.equal(d_cup, d_cup2)
    t_pt, t_cup = R.logbinom_bwd(pt.cpu().to(F64), cen.cpu().to(F64), gd.cpu().to(F64), 0.0212, 50.0)
    p = pt.clone().requires_grad_(True)
    cu = pf_oracle.up(cen.permute(0, 3, 1, 2), (9, 13)).permute(0, 2, 3, 1).detach().requires_grad_(True)    # (the oracle's float32 up-sampling)
    R.logbinom_fwd_up(p, cu, 0.0212, 50.0).backward(gd)
    hold("logbinom_bwd d_pt", d_pt, t_pt, p.grad)
    hold("logbinom_bwd d_centers_up", d_cup, t_cup, cu.grad)
    # the forward kernel agrees with the restated forward the truth differentiates
    depth = torch.empty(2, 9, 13, device=DEV)
    ops.logbinom_depth(ptb[..., :4], cen, depth, 0.0212, 50.0)
    want = R.logbinom_fwd(pt.cpu().to(F64), cen.cpu().to(F64), 0.0212, 50.0)
    assert normwise(depth, want) <= 1e-5


# ---------------- activations ----------------
@pytest.mark.parametrize("act", ["relu", "softplus", "gelu"])
def test_act_backward(ops, act):
    g = torch.Generator().manual_seed(23)
    z = (torch.randn(2, 5, 7, 16, generator=g) * 2).to(DEV)[..., :12].requires_grad_(True)
    gy = torch.randn(2, 5, 7, 12, generator=g).to(DEV)
    y = {"relu": torch.relu, "softplus": F.softplus, "gelu": F.gelu}[act](z)
    y.backward(gy)
    ref = z.detach() if act == "gelu" else y.detach()
    got, got2 = ops.act_bwd(gy.clone(), ref, act), ops.act_bwd(gy.clone(), ref, act)
    assert torch.equal(got, got2)
    hold(f"act_bwd {act}", got, R.act_bwd(gy.cpu().to(F64), ref.cpu().to(F64), act), z.grad)


# ---------------- SILog ----------------
@pytest.mark.parametrize("case", ["partial", "one_valid", "other_grid"])
def test_silog_backward(ops, case):
    g = torch.Generator().manual_seed(29)
    ph, pw = (5, 7) if case == "other_grid" else (9, 13)
    pred = (torch.rand(2, 1, ph, pw, generator=g) * 60 + 1).to(DEV)
    target = (torch.rand(2, 1, 9, 13, generator=g) * 100 - 5).to(DEV)
    if case == "one_valid":
        target = torch.full_like(target, -1.0)
        target[1, 0, 4, 6] = 10.0
    lo, hi = 1e-3, 80.0

    def run():
        up = pf_oracle.up(pred, (9, 13)).contiguous() if case == "other_grid" else pred
        loss, sums = ops.silog_loss_saved(up, target, lo, hi)
        d_up = ops.silog_loss_bwd(up, target, sums, nan_like(tuple(up.shape)), lo, hi)
        if case != "other_grid":
            return loss, d_up
        return loss, ops.resize_bwd(d_up.view(2, 9, 13, 1), nan_like((2, ph, pw, 1))).view(2, 1, ph, pw)

    (loss, d), (_, d2) = run(), run()
    assert torch.equal(d, d2)

    def autograd(dtype, dev):
        p = pred.to(device=dev, dtype=dtype).requires_grad_(True)
        l = pf_oracle.silog_loss(p, target.to(device=dev, dtype=dtype), lo, hi)
        l.sum().backward()
        return l.detach(), p.grad

    l64, truth = autograd(F64, "cpu")
    if case == "one_valid":
        assert not d.any() and not truth.any() and float(loss) == 0.0
        return
    _, comp = autograd(torch.float32, DEV)
    assert int((truth != 0).sum()) < truth.numel() or case == "other_grid"
    hold(f"silog_bwd {case}", d, truth, comp)
    assert abs(float(loss) - float(l64)) <= 1e-5 * float(l64)
