"""The bar of tests/test_bf16_grade_gpu.py has teeth (f64_ref.bf16_excess / bf16_grade): no GPU needed.

The model of a bf16 kernel is what csrc/igemm.hip does: bf16 operands (exact), float32 accumulation, the epilogue in float32 through bias and
residual, ONE rounding to nearest even on the store.  The bar accepts it with a margin of at least 10x and refuses each way such a kernel goes
subtly wrong; the normwise 2e-2 bar of tests/op_checks.py accepts three of them, which is the gap the element-wise module closes."""
import pytest
import torch
import torch.nn.functional as F

from tests import f64_ref as R

BF = torch.bfloat16


def _bf(t):
    return t.to(BF)


def _trunc_bf16(v):
    """float32 -> bfloat16 by dropping the low 16 bits (round toward zero)"""
    return (v.float().contiguous().view(torch.int32) & -65536).view(torch.float32).to(BF)


def _passes(y, ref, mag, base, margin=1.0):
    e = R.bf16_excess(y, ref, mag)
    return R.bf16_grade((e[0] * margin, e[1] * margin), base), e


def _linear(K, res=True, cols=False, M=400, N=96):
    g = torch.Generator().manual_seed(K)
    x = _bf(torch.randn(M, K, generator=g))
    w = torch.randn(N, K, generator=g) / K ** 0.5
    b = torch.randn(N, generator=g)
    if cols:                                   # column 5 at 1e-3 of the others, through its weight row and its bias
        w[5] *= 1e-3
        b[5] *= 1e-3
    w = _bf(w)
    r = _bf(torch.randn(M, N, generator=g)) if res else None
    ref, mag = R.linear_ref(x, w, b, res=r)
    return x, w, b, r, ref, mag


@pytest.mark.parametrize("K", [128, 1152, 4896])
def test_linear_model_passes_with_margin_and_every_mutation_fails(K):
    x, w, b, r, ref, mag = _linear(K)
    acc = x.float() @ w.float().t() + b
    base = R.errors(acc + r.float(), ref, mag)                 # the float32 result before the store: the baseline of the bar
    good = _bf(acc + r.float())
    ok, e = _passes(good, ref, mag, base, margin=10.0)
    assert ok, (K, e, base)
    assert R.bf16_grade(R.errors(acc + r.float(), ref, mag), base)           # an out_f32 output: the plain element-wise error
    dropped = _bf(x[:, :K - 32].float() @ w[:, :K - 32].float().t() + b + r.float())
    double = _bf(_bf(acc).float() + r.float())
    trunc = _trunc_bf16(acc + r.float())
    for name, y in (("one 32-wide K chunk dropped", dropped), ("rounded before the residual add", double), ("truncated", trunc)):
        ok, e = _passes(y, ref, mag, base)
        assert not ok and e[0] >= 1e-4, (K, name, e)
    # the gap: the normwise 2e-2 bar accepts the second rounding and the truncation
    assert R.old_normwise_bar(double, ref, tol=2e-2) and R.old_normwise_bar(trunc, ref, tol=2e-2)
    assert R.old_normwise_bar(good, ref, tol=2e-2)


@pytest.mark.parametrize("K", [128, 1152, 4896])
def test_bias_missing_in_one_small_column_fails_and_passes_the_old_bar(K):
    x, w, b, _, ref, mag = _linear(K, res=False, cols=True)
    acc = x.float() @ w.float().t()
    base = R.errors(acc + b, ref, mag)
    ok, e = _passes(_bf(acc + b), ref, mag, base, margin=10.0)
    assert ok, (K, e, base)
    assert float(ref[:, 5].abs().max()) <= 2e-3 * float(ref.abs().max())
    b_bad = b.clone()
    b_bad[5] = 0
    bad = _bf(acc + b_bad)
    ok, e = _passes(bad, ref, mag, base)
    assert not ok and e[0] >= 1e-3, (K, e)         # (|b| against mag = sum |w||x| + |b|, which grows like sqrt(K))
    assert R.old_normwise_bar(bad, ref, tol=2e-2)


def _conv3x3(x, w, b):
    """float32 3x3 / pad 1 convolution of NHWC x with w [N, C, 3, 3]"""
    return F.conv2d(x.float().permute(0, 3, 1, 2), w.float(), b, padding=1).permute(0, 2, 3, 1)


def test_conv_model_passes_and_one_clamped_border_tap_fails():
    g = torch.Generator().manual_seed(9)
    B, H, W, C, N = 2, 9, 13, 32, 24
    x = _bf(torch.randn(B, H, W, C, generator=g))
    w = _bf(torch.randn(N, C, 3, 3, generator=g) / (9 * C) ** 0.5)
    b = torch.randn(N, generator=g)
    r = _bf(torch.randn(B, H, W, N, generator=g))
    pix = R.sample_pixels(B, H, W, n_random=64, seed=1, tile=4)
    ref, mag = R.conv_ref(x, w, pix, b, 1, 1, res=r)
    acc = _conv3x3(x, w, b) + r.float()
    base = R.errors(R.gather_pixels(acc, pix, N), ref, mag)
    good = _bf(acc)
    ok, e = _passes(R.gather_pixels(good, pix, N), ref, mag, base, margin=10.0)
    assert ok, (e, base)
    # output pixel (b 1, oy 0, ox 4): tap (ky 0, kx 1) lies in the zero padding; the mutation reads the clamped neighbour x[1, 0, 4]
    assert (pix == torch.tensor([1, 0, 4])).all(1).any()
    wrong = acc.clone()
    wrong[1, 0, 4] += w[:, :, 0, 1].float() @ x[1, 0, 4].float()
    ok, e = _passes(R.gather_pixels(_bf(wrong), pix, N), ref, mag, base)
    assert not ok and e[0] >= 1e-3, e
    for name, y in (("rounded before the residual add", _bf(_bf(acc - r.float()).float() + r.float())), ("truncated", _trunc_bf16(acc))):
        ok, e = _passes(R.gather_pixels(y, pix, N), ref, mag, base)
        assert not ok, (name, e)


def test_excess_is_zero_for_a_correctly_rounded_value_and_inf_for_nan():
    ref = torch.tensor([[1.0 + 2.0 ** -9, 3.0, -0.7]], dtype=torch.float64)
    y = _bf(ref.float())
    assert R.bf16_excess(y, ref, ref.abs())[0] == 0.0
    assert R.bf16_excess(torch.full((1, 3), float("nan"), dtype=BF), ref, ref.abs())[0] == float("inf")
    # one bf16 ulp off (a wrong rounding direction): half an ulp beyond the storage rounding
    up = (y.view(torch.int16) + 1).view(BF)
    assert R.bf16_excess(up, ref, ref.abs())[0] >= 2.0 ** -10
