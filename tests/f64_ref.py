"""Sampled float64 reference of the NHWC convolutions / linears and the element-wise error metric of the float32-grade checks
(tests/test_float32_grade_gpu.py; CPU checks of the reference itself in tests/test_f64_ref_cpu.py) and of the bf16-grade checks
(tests/test_bf16_grade_gpu.py: bf16_excess / bf16_grade, proved on the CPU in tests/test_bf16_grade_ref_cpu.py).  No GPU needed.

The reference evaluates the layer in float64 on the CPU at a chosen set of output pixels (rows of a linear), every output channel, in the epilogue
order of tests/fake_ops.py: bias -> act -> scale -> res -> res2.  Next to it comes the magnitude of every element,

    mag = |s| (L (sum |w||x| + |b|) [+ |softplus(v)|]) + |res| + |res2|          (L: Lipschitz factor of the activation; 1.13 for GELU)

which bounds what a float32-grade kernel may get wrong in that element: the element-wise error max |y - ref| / mag sees a wrong power-of-two
scale of one output column or one input channel at 1e-4 of the largest value, which the normwise error max |y - ref| / max |ref| cannot.
(Softplus adds |softplus(v)| itself: softplus(0) = log 2 is not bounded by the Lipschitz term.)"""
import math

import torch
import torch.nn.functional as F

GELU_LIPSCHITZ = 1.1289          # max |GELU'(z)| (z = +-0.7518)
TINY = torch.finfo(torch.float32).tiny


def _act(v, act):
    if act in (None, "none"):
        return v
    if act == "relu":
        return torch.relu(v)
    if act == "gelu":
        return F.gelu(v)
    if act == "softplus":
        return F.softplus(v)
    raise ValueError(act)


def _epilogue(z, zmag, bias, act, scale, res, res2):
    """z = float64 products [P, N], zmag = sum |w||x| [P, N]; res / res2 float64 [P, N] at the same elements"""
    v = z if bias is None else z + bias
    bmag = zmag if bias is None else zmag + bias.abs()
    a = _act(v, act)
    mag = bmag * (GELU_LIPSCHITZ if act == "gelu" else 1.0)
    if act == "softplus":
        mag = mag + a.abs()
    if scale is not None:
        a, mag = a * scale, mag * scale.abs()
    for r in (res, res2):
        if r is not None:
            a, mag = a + r, mag + r.abs()
    return a, mag


def _d(t, n=None):
    if t is None:
        return None
    t = t.detach().cpu().double()
    return t[..., :n] if n is not None else t


def linear_ref(x, w, bias=None, act=None, scale=None, res=None, res2=None, rows=None, relu_in=False):
    """x [M, K] (any float dtype, any device), w [N, K]; res / res2 [M, >= N]; rows: LongTensor of the rows to evaluate (None: all).
    -> (ref, mag), float64 [len(rows), N]"""
    N = w.shape[0]
    rows = torch.arange(x.shape[0]) if rows is None else rows
    xs = x[rows.to(x.device)].detach().cpu().double()
    if relu_in:
        xs = xs.clamp_min(0)
    wd = _d(w)
    z, zmag = xs @ wd.t(), xs.abs() @ wd.abs().t()
    pick = lambda r: None if r is None else r[rows.to(r.device)].detach().cpu().double()[:, :N]
    return _epilogue(z, zmag, _d(bias, N), act, _d(scale, N), pick(res), pick(res2))


def conv_ref(x, w, pix, bias=None, stride=1, pad=0, act=None, relu_in=False, scale=None, res=None, res2=None):
    """x NHWC [B, H, W, >= Cin] (channel-slice views fine), w [N, Cin, KH, KW]; pix LongTensor [P, 3] of output pixels (b, oy, ox);
    res / res2 NHWC [B, OH, OW, >= N].  -> (ref, mag), float64 [P, N]"""
    N, Cin, KH, KW = w.shape
    B, H, W, _ = x.shape
    b, oy, ox = (pix[:, i] for i in range(3))
    z = torch.zeros(pix.shape[0], N, dtype=torch.float64)
    zmag = torch.zeros_like(z)
    wd = _d(w)
    for ky in range(KH):
        for kx in range(KW):
            iy, ix = oy * stride - pad + ky, ox * stride - pad + kx
            ok = (iy >= 0) & (iy < H) & (ix >= 0) & (ix < W)
            g = x[b.to(x.device), iy.clamp(0, H - 1).to(x.device), ix.clamp(0, W - 1).to(x.device), :Cin].detach().cpu().double()
            g = g * ok[:, None]
            if relu_in:
                g = g.clamp_min(0)
            wt = wd[:, :, ky, kx]
            z += g @ wt.t()
            zmag += g.abs() @ wt.abs().t()
    pick = lambda r: None if r is None else r[b.to(r.device), oy.to(r.device), ox.to(r.device)].detach().cpu().double()[:, :N]
    return _epilogue(z, zmag, _d(bias, N), act, _d(scale, N), pick(res), pick(res2))


def conv_transpose_ref(x, w, pix, bias=None):
    """nn.ConvTranspose2d(kernel = stride = s, padding 0) on NHWC x [B, H, W, >= Cin], w [Cin, Cout, s, s] (packing.pack_conv_transpose):
    out[b, y s + dy, x s + dx, co] = bias[co] + sum_ci x[b, y, x, ci] w[ci, co, dy, dx].  pix = output pixels of the s-times larger image."""
    Cin, N, s, _ = w.shape
    b, oy, ox = (pix[:, i] for i in range(3))
    g = x[b.to(x.device), (oy // s).to(x.device), (ox // s).to(x.device), :Cin].detach().cpu().double()    # [P, Cin]
    wt = _d(w)[:, :, oy % s, ox % s].permute(2, 1, 0)                                                        # [P, N, Cin]
    z = torch.einsum("pc,pnc->pn", g, wt)
    zmag = torch.einsum("pc,pnc->pn", g.abs(), wt.abs())
    return _epilogue(z, zmag, _d(bias, N), None, None, None, None)


def errors(y, ref, mag):
    """(element-wise, normwise) error of y [P, N] (any device / dtype) against the float64 ref / mag of the same elements; inf when y is not finite"""
    y = y.detach().cpu().double()
    if not torch.isfinite(y).all():
        return float("inf"), float("inf")
    d = (y - ref).abs()
    return float((d / (mag + TINY)).max()), float(d.max() / max(float(ref.abs().max()), TINY))


def gather_pixels(y, pix, n):
    """the n output channels of NHWC y at the output pixels pix [P, 3]"""
    dev = y.device
    return y[pix[:, 0].to(dev), pix[:, 1].to(dev), pix[:, 2].to(dev), :n]


def float32_grade(e, base, norm_cap, elem_cap):
    """the bar of the float32-grade checks: e = (element-wise, normwise) of the route, base = the same of the float32 baseline on the same operands.
    Each at most twice the baseline's, normwise <= norm_cap, element-wise <= elem_cap."""
    return e[0] <= 2 * base[0] and e[1] <= 2 * base[1] and e[1] <= norm_cap and e[0] <= elem_cap


def bf16_excess(y, ref, mag):
    """what a stored output y [P, N] is off by beyond its own storage rounding, as (element-wise, normwise) like errors().  A bfloat16 y is a float32
    value v rounded once to nearest, and a v that rounds to y lies within half a bfloat16 ulp of y (f64_image_ref.bf16_half_ulp, evaluated at the
    STORED value), so

        excess = max(0, |y - ref| - half_ulp_bf16(y)) / mag

    is a lower bound of |v - ref| / mag: ~1e-8 for a float32-accumulated product rounded once, >= 3e-4 for a second rounding before a residual
    add, for truncation, for a dropped K chunk (tests/test_bf16_grade_ref_cpu.py).  A float32 y (out_f32) has no storage rounding: errors()."""
    if y.dtype != torch.bfloat16:
        return errors(y, ref, mag)
    from tests.f64_image_ref import bf16_half_ulp
    y = y.detach().cpu().double()
    if not torch.isfinite(y).all():
        return float("inf"), float("inf")
    d = ((y - ref).abs() - bf16_half_ulp(y)).clamp_min(0)
    return float((d / (mag + TINY)).max()), float(d.max() / max(float(ref.abs().max()), TINY))


BASE_FLOOR = 4 * 2.0 ** -24      # floor of a baseline's error (f64_image_ref.baseline_bar: one stray rounding in the baseline must not decide)


def bf16_grade(e, base, elem_cap=None):
    """the bar of the bf16-grade checks (tests/test_bf16_grade_gpu.py), after float32_grade: e = bf16_excess of the bf16 kernel, base = errors() of the
    float32-MFMA kernel on the same bf16-valued operands.  The largest element-wise excess at most ELEM_CAP_GEMM and at most twice the baseline's
    element-wise error, the baseline floored at 4 * 2^-24.  (No cap comes from the bf16 kernels' own measured error.)"""
    cap = ELEM_CAP_GEMM if elem_cap is None else elem_cap
    return e[0] <= cap and e[0] <= 2 * max(base[0], BASE_FLOOR)


def old_normwise_bar(y, ref, tol=2e-4):
    """tests/op_checks.py's bar: max |y - ref| / max(1, max |ref|) <= 2e-4"""
    y = y.detach().cpu().double()
    if not torch.isfinite(y).all():
        return False
    return float((y - ref).abs().max()) / max(1.0, float(ref.abs().max())) <= tol


# ---------------- samplers ----------------

def _seams(n, tile=4):
    """coordinates in [0, n): the borders, the seams of the first Winograd tiles (mod 4 in {0, 3}), the ragged last tile and the middle"""
    last = (n - 1) // tile * tile
    c = {0, 1, 3, 4, 7, 8, last - 1, last, n - 2, n - 1, n // 2, n // 2 // tile * tile - 1, n // 2 // tile * tile}
    return sorted(v for v in c if 0 <= v < n)


def sample_pixels(B, OH, OW, n_random=256, seed=0, window=None, tile=4):
    """LongTensor [P, 3] of output pixels (b, oy, ox): the seam grid (borders, Winograd tile seams, ragged last tile row / column) of the first and
    the last batch image, the corners of the tiles either side of every window seam (window = tiles per window of hip_ops.wino3_window, tiles
    numbered b TH TW + ty TW + tx), and n_random seeded random pixels."""
    pts = set()
    ys, xs = _seams(OH, tile), _seams(OW, tile)
    for b in sorted({0, B - 1}):
        pts.update((b, y, x) for y in ys for x in xs)
    TH, TW = -(-OH // tile), -(-OW // tile)
    T = B * TH * TW
    if window is not None and window < T:
        for t0 in range(window, T, window):
            for t in (t0 - 1, t0):
                b, r = divmod(t, TH * TW)
                ty, tx = divmod(r, TW)
                for dy, dx in ((0, 0), (tile - 1, tile - 1), (0, tile - 1)):
                    pts.add((b, min(ty * tile + dy, OH - 1), min(tx * tile + dx, OW - 1)))
    g = torch.Generator().manual_seed(seed)
    r = torch.stack([torch.randint(0, B, (n_random,), generator=g), torch.randint(0, OH, (n_random,), generator=g),
                     torch.randint(0, OW, (n_random,), generator=g)], 1)
    pts.update(map(tuple, r.tolist()))
    return torch.tensor(sorted(pts), dtype=torch.long)


def sample_rows(M, n_random=256, seed=0):
    """LongTensor of linear rows: 0, 1, every multiple of 64 / 128 / 192 / 256 and its neighbours, the ragged tail (the last 8 rows and the
    first row of every partial last block) and n_random seeded random rows"""
    rows = {0, 1}
    for t in (64, 128, 192, 256):
        for m in range(t, M + 1, t):
            rows.update((m - 1, m, m + 1))
        rows.add(M // t * t)
    rows.update(range(max(0, M - 8), M))
    g = torch.Generator().manual_seed(seed)
    rows.update(torch.randint(0, M, (n_random,), generator=g).tolist())
    return torch.tensor(sorted(r for r in rows if 0 <= r < M), dtype=torch.long)


def pixel_rows(B, OH, OW, pix):
    """flat row index b OH OW + oy OW + ox of the pixels"""
    return (pix[:, 0] * OH + pix[:, 1]) * OW + pix[:, 2]


def decade_spread(n, lo, hi, seed):
    """n float64 factors 10^u, u uniform in [log10 lo, log10 hi] (seeded)"""
    g = torch.Generator().manual_seed(seed)
    return 10.0 ** (math.log10(lo) + torch.rand(n, generator=g, dtype=torch.float64) * (math.log10(hi) - math.log10(lo)))


# ---------------- bars (tests/test_float32_grade_gpu.py; measured values: profiles/r9_float32_grade.log) ----------------
NORM_CAP_GEMM = 2e-6          # normwise, 1x1 / linear routes: the bar of op_checks.gemm_split3 / conv1x1_split3
NORM_CAP_WINO = 3.2e-5        # normwise, Winograd routes: the bar of op_checks.conv_winograd_fused
# element-wise caps = 4x the worst measured (profiles/r9_float32_grade.log)
ELEM_CAP_GEMM = 2.3e-6        # 1x1 / linear / direct routes and the LayerNorm producers: worst 5.7e-7 (LayerNorm planes, = the f32 kernel)
ELEM_CAP_WINO = 2.4e-3        # Winograd routes: worst 6.1e-4 (fused, spike pixels at 1e3x spread their rounding over the tile; f32 three-step 4.2e-4)
