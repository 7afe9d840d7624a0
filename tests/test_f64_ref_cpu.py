"""CPU checks of the sampled float64 reference (tests/f64_ref.py) and of its power to fail kernels: at every sampled element it equals a full
float64 convolution; emulated kernel bugs (bf16x3 without its h.m / m.h terms, fp16x2 without h.l, one column or input-channel exponent off by one,
the ragged last row block unwritten) fail the bars of tests/test_float32_grade_gpu.py while an honest float32 computation passes them.  Also the
layout rule of the s3_1x1 route (hip_ops.conv1x1_split3_layout_ok) on unaligned layouts."""
import pytest
import torch
import torch.nn.functional as F

from patchfusion_amd import packing as pk
from tests import f64_ref as R


def _full_conv(x, w, bias, stride, pad, act, relu_in, scale, res, res2):
    xd = x.double().permute(0, 3, 1, 2)
    if relu_in:
        xd = xd.clamp_min(0)
    v = F.conv2d(xd, w.double(), None if bias is None else bias.double(), stride=stride, padding=pad).permute(0, 2, 3, 1)
    v = R._act(v, act)
    if scale is not None:
        v = v * scale.double()
    for r in (res, res2):
        if r is not None:
            v = v + r.double()[..., :w.shape[0]]
    return v


@pytest.mark.parametrize("k,stride,pad,act,relu_in,epi", [
    (3, 1, 1, "relu", True, True), (3, 2, 1, None, False, True), (1, 1, 0, "gelu", False, True), (1, 1, 0, "softplus", True, False),
    (3, 1, 1, None, False, False)])
def test_sampled_conv_equals_full_float64_conv(k, stride, pad, act, relu_in, epi):
    g = torch.Generator().manual_seed(k * 10 + stride)
    B, H, W, cin, cout = 2, 19, 23, 24, 20
    xb = torch.randn(B, H, W, cin + 8, generator=g)
    x = xb[..., 4:4 + cin]                                           # a channel-slice view
    w = torch.randn(cout, cin, k, k, generator=g)
    b = torch.randn(cout, generator=g)
    OH, OW = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    sc = torch.rand(cout, generator=g) + 0.5 if epi else None
    r1 = torch.randn(B, OH, OW, cout + 4, generator=g) if epi else None
    r2 = torch.randn(B, OH, OW, cout, generator=g) if epi else None
    full = _full_conv(x, w, b, stride, pad, act, relu_in, sc, r1, r2)
    pix = R.sample_pixels(B, OH, OW, n_random=64, seed=1)
    ref, mag = R.conv_ref(x, w, pix, b, stride, pad, act, relu_in, sc, r1, r2)
    want = full[pix[:, 0], pix[:, 1], pix[:, 2]]
    assert torch.allclose(ref, want, rtol=1e-12, atol=1e-12)
    assert bool((mag >= want.abs() * (1 - 1e-12)).all()) or act == "softplus"
    assert R.errors(want, ref, mag)[0] < 1e-12


@pytest.mark.parametrize("s", [2, 4])
def test_sampled_transposed_conv_equals_full_float64(s):
    g = torch.Generator().manual_seed(s)
    x = torch.randn(2, 5, 7, 16, generator=g)
    w = torch.randn(16, 12, s, s, generator=g)
    b = torch.randn(12, generator=g)
    full = F.conv_transpose2d(x.double().permute(0, 3, 1, 2), w.double(), b.double(), stride=s).permute(0, 2, 3, 1)
    pix = R.sample_pixels(2, 5 * s, 7 * s, n_random=32, seed=2)
    ref, _ = R.conv_transpose_ref(x, w, pix, b)
    assert torch.allclose(ref, full[pix[:, 0], pix[:, 1], pix[:, 2]], rtol=1e-12, atol=1e-12)


def test_linear_ref_equals_full_and_rows_cover_the_tiles():
    g = torch.Generator().manual_seed(3)
    M, K, N = 1037, 64, 40
    x, w, b = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g), torch.randn(N, generator=g)
    res = torch.randn(M, N + 4, generator=g)
    rows = R.sample_rows(M, n_random=16)
    ref, _ = R.linear_ref(x, w, b, "gelu", None, res, None, rows)
    full = F.gelu(x.double() @ w.double().t() + b.double()) + res.double()[:, :N]
    assert torch.allclose(ref, full[rows], rtol=1e-12, atol=1e-12)
    got = set(rows.tolist())
    for t in (64, 128, 192, 256):
        assert {t - 1, t, t + 1, M // t * t} <= got
    assert set(range(M - 8, M)) <= got


def test_pixel_sampler_covers_borders_seams_and_windows():
    B, OH, OW = 3, 37, 45
    pix = R.sample_pixels(B, OH, OW, n_random=8, seed=0, window=24)
    pts = set(map(tuple, pix.tolist()))
    for b in (0, B - 1):
        for y in (0, OH - 1, 3, 4, 36 // 4 * 4):                     # borders, tile seams, the ragged last tile row
            for x in (0, OW - 1, 3, 4, 44 // 4 * 4):
                assert (b, y, x) in pts
    TW = -(-OW // 4)
    tiles = {b * (-(-OH // 4)) * TW + (y // 4) * TW + x // 4 for b, y, x in pts}
    T = B * (-(-OH // 4)) * TW
    for t0 in range(24, T, 24):                                      # both tiles either side of every window seam
        assert t0 - 1 in tiles and t0 in tiles
    assert bool((pix[:, 1] < OH).all() and (pix[:, 2] < OW).all())


# ---------------- mutant controls ----------------

def _layer(M, K, N, seed, col_scale=None, in_scale=None):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, K, generator=g, dtype=torch.float64)
    w = torch.randn(N, K, generator=g, dtype=torch.float64) / K ** 0.5
    b = torch.randn(N, generator=g, dtype=torch.float64)
    if in_scale is not None:
        x, w = x * in_scale, w / in_scale
    if col_scale is not None:
        w, b = w * col_scale[:, None], b * col_scale
    return x.float(), w.float(), b.float()


def _f32(x, w, b):
    return x @ w.t() + b                                            # honest float32 (torch CPU GEMM)


def _split3_product(x, w, b, terms):
    xs, ws = pk.split3(x), pk.split3(w)
    acc = sum(xs[i].double() @ ws[j].double().t() for i, j in terms)
    return (acc + b.double()).float()


def _f16x2_product(x, w, b, terms):
    bound = x.double().abs().amax(0)
    pw = pk.pack_conv_f16x2(w, b, None, bound)
    xs = pk.split_f16x2(torch.ldexp(x.double(), -pw.in_exp.double()[None, :]).float())
    ws = pk.kmajor_to_rows(pw.w)[:, :w.shape[0]]
    acc = sum(xs[i].double() @ ws[j].double().t() for i, j in terms)
    return (torch.ldexp(acc, pw.col_exp[:w.shape[0]].double()[None, :]) + b.double()).float()


def _bars(y, x, w, b, rows=None, cap=R.NORM_CAP_GEMM):
    ref, mag = R.linear_ref(x, w, b, rows=rows)
    base = R.errors(_f32(x, w, b)[rows if rows is not None else slice(None)], ref, mag)
    e = R.errors(y[rows] if rows is not None else y, ref, mag)
    return R.float32_grade(e, base, cap, R.ELEM_CAP_GEMM), e, base


BF16X3_TERMS = [(0, 0), (0, 1), (1, 0), (0, 2), (2, 0), (1, 1)]
F16X2_TERMS = [(0, 0), (0, 1), (1, 0)]


def test_honest_split_products_pass_and_dropped_terms_fail():
    x, w, b = _layer(300, 256, 96, 1)
    ok, e, base = _bars(_split3_product(x, w, b, BF16X3_TERMS), x, w, b)
    assert ok, (e, base)
    ok, e, base = _bars(_f16x2_product(x, w, b, F16X2_TERMS), x, w, b)
    assert ok, (e, base)
    ok, e, _ = _bars(_split3_product(x, w, b, [t for t in BF16X3_TERMS if t not in ((0, 1), (1, 0))]), x, w, b)
    assert not ok, e                                                 # bf16x3 without h.m and m.h
    ok, e, _ = _bars(_f16x2_product(x, w, b, [(0, 0), (1, 0)]), x, w, b)
    assert not ok, e                                                 # fp16x2 without h.l


def test_column_exponent_off_by_one_passes_the_old_bar_and_fails_the_element_wise_bar():
    N, n_bad = 96, 37
    cs = torch.ones(N, dtype=torch.float64)
    cs[n_bad] = 1e-4                                                 # one output column at 1e-4 of the others
    x, w, b = _layer(300, 256, N, 2, col_scale=cs)
    y = _f32(x, w, b)
    assert _bars(y, x, w, b)[0]
    bad = y.clone()
    bad[:, n_bad] *= 2                                               # its exponent f_n off by one
    ref, mag = R.linear_ref(x, w, b)
    assert R.old_normwise_bar(bad, ref), "the old normwise 2e-4 bar must not see this (the gap the element-wise bar closes)"
    ok, e, base = _bars(bad, x, w, b)
    assert not ok and e[0] > 0.1, (e, base)


def test_input_channel_exponent_off_by_one_fails():
    K, k_bad = 256, 101
    s = torch.ones(K, dtype=torch.float64)
    s[k_bad] = 1e-3                                                  # one input channel at 1e-3 scale, its weights compensate
    x, w, b = _layer(300, K, 96, 3, in_scale=s)
    assert _bars(_f32(x, w, b), x, w, b)[0]
    xb = x.clone()
    xb[:, k_bad] *= 2                                                # its exponent e_k off by one
    ok, e, _ = _bars(_f32(xb, w, b), x, w, b)
    assert not ok, e


@pytest.mark.parametrize("tile", [64, 192])
def test_unwritten_ragged_last_row_block_fails(tile):
    M = 1037
    x, w, b = _layer(M, 64, 32, 4)
    y = _f32(x, w, b)
    rows = R.sample_rows(M, n_random=8)
    assert _bars(y, x, w, b, rows)[0]
    bad = y.clone()
    bad[M // tile * tile:] = float("nan")                            # (the GPU checks fill their outputs with NaN before the launch)
    ok, e, _ = _bars(bad, x, w, b, rows)
    assert not ok and e[0] == float("inf")


# ---------------- the s3_1x1 layout rule ----------------

def _pw1x1(cin=64, cout=80, scale=False):
    w = torch.randn(cout, cin, 1, 1)
    return pk.pack_conv(w, torch.randn(cout), dtype=torch.float32, scale=torch.rand(cout) if scale else None)


def test_conv1x1_split3_layout_rule():
    from patchfusion_amd.hip_ops import conv1x1_split3_layout_ok as ok
    pw = _pw1x1(scale=True)
    assert pw.w3 is not None
    A = 1 << 20                                                      # a 16-byte aligned base address
    assert ok(pw, A, 64, A + 4096, 80)
    assert ok(pw, A, 64, A + 4096, 80, A + 8192, 84, A + 16384, 80)
    assert not ok(pw, A + 4, 64, A + 4096, 80)                       # x one float off
    assert not ok(pw, A, 64, A + 4100, 80)                           # y one float off
    assert not ok(pw, A, 64, A + 4096, 80, A + 8196, 84)             # res one float off (a view res[..., 1:])
    assert not ok(pw, A, 64, A + 4096, 80, None, 0, A + 8200, 84)    # res2 two floats off
    assert not ok(pw, A, 66, A + 4096, 80)                           # x_ld not a multiple of 4
    assert not ok(pw, A, 64, A + 4096, 80, A + 8192, 82)             # res_ld not a multiple of 4
    assert not ok(pw, A, 32, A + 4096, 80)                           # x_ld < Cin
    pw.bias = pw.bias[1:]                                            # a bias one float off
    assert not ok(pw, A, 64, A + 4096, 80)


def test_conv_plan_key_carries_pointer_alignment():
    from patchfusion_amd.hip_ops import _align16
    buf = torch.zeros(2, 3, 5, 88)
    assert _align16(buf[..., :80], None) != _align16(buf[..., 1:81], None)
    assert _align16(buf[..., :80], None) == _align16(buf[..., 4:84], None)
