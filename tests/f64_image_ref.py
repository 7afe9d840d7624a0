"""Float64 references and per-element magnitudes of the non-GEMM kernels (csrc/imageops.hip, csrc/swin.hip): bilinear / nearest resize, crop-resize,
roi_align, maxpool2, the tile stitcher, the Swin (G2L) partition / window attention / reverse, and the attractor / log-binomial kernels of the
metric-bins head, the fused metric-bins tail and the seed / bounded bin centres.  Style and metric of tests/f64_ref.py; used by
tests/test_image_grade_gpu.py and tests/test_tail_grade_gpu.py, checked on the CPU by tests/test_f64_image_ref_cpu.py.  No GPU needed.

Every function takes the operands the kernel sees (float32 tensors, or bf16 tensors read as their exact values; scalar arguments as the float32 the
C ABI passes) and returns (ref, mag) in float64 for EVERY output element.  What the operation defines in float32 is evaluated in float32 here too:
the source coordinate of a resize (PyTorch: scale = fl((in-1)/(out-1)), src = fl(scale * dst); csrc/imageops.hip ac_coord), the sample coordinates
of roi_align (torchvision's operation order) and the arguments k + 1e-7, n - k + 1e-7 of the log-binomial's Stirling terms.  These select taps and
weights; the weights themselves (l1 = src - floor(src) is exact), the blends, sums, divisions, exponentials and logarithms are float64.

mag is the sum of the absolute values of the terms of an element: a float32 kernel with k roundings on its longest path is off by at most
k 2^-24 mag (first order), so max |y - ref| / mag sees one wrong tap, weight, bin or mask entry that max |y - ref| / max |ref| hides."""
import math

import numpy as np
import torch

from tests.f64_ref import TINY, errors            # noqa: F401  (errors: the (element-wise, normwise) pair of y against ref / mag)

U = 2.0 ** -24                   # float32 unit roundoff
FLOOR = 4 * U                    # floor of a baseline's error in baseline_bar
WIN = 12
f32 = np.float32

# roundings on the longest path of an element (derivations: tests/test_image_grade_gpu.py)
K_BILERP, K_BILERP_ADD, K_STITCH_INIT, K_DIV, K_STITCH_AVG, K_ADD = 6, 7, 1, 1, 4, 1


def _d(t):
    return t.detach().cpu().double()


# ---------------- bars ----------------
def bf16_half_ulp(v):
    """half a bfloat16 ulp at |v| (float64): 2^(floor(log2 |v|) - 8) -- bfloat16 keeps 8 significant bits, so rounding to nearest moves a value by
    at most this; between 2^-9 |v| (top of a binade) and 2^-8 |v| (bottom)"""
    _, e = torch.frexp(v.abs())
    return torch.where(v != 0, torch.ldexp(torch.ones_like(v), e - 9), torch.zeros_like(v))


def counted_bar(y, ref, mag, k, bf16_out=False):
    """|y - ref| <= k 2^-24 mag at every element; a bf16 output adds its one rounding to nearest, half a bf16 ulp of the float32 value rounded
    (|ref| + k 2^-24 mag at most) -> (ok, worst |y - ref| / bound; inf when y is not finite)"""
    y = _d(y)
    if not torch.isfinite(y).all():
        return False, float("inf")
    bound = k * U * mag
    if bf16_out:
        bound = bound + bf16_half_ulp(ref.abs() + bound)
    d = (y - ref).abs()
    ok = bool((d <= bound).all())
    worst = float((d / (bound + TINY)).max()) if d.numel() else 0.0
    return ok, worst


def baseline_bar(e, base):
    """e, base = errors() of the kernel and of the float32 restatement on the same operands: each of the kernel's at most twice the baseline's,
    the baseline floored at 4 * 2^-24 (one stray rounding in the baseline must not decide)"""
    return e[0] <= 2 * max(base[0], FLOOR) and e[1] <= 2 * max(base[1], FLOOR)


# ---------------- bilinear resize, align_corners=True ----------------
def ac_scale(n_in, n_out):
    return f32(n_in - 1) / f32(n_out - 1) if n_out > 1 else f32(0)


def ac_taps(n_in, n_out):
    """-> i0, i1 (LongTensor [n_out]), l1 (float64 [n_out], the exact float32 difference src - i0)"""
    src = ac_scale(n_in, n_out) * np.arange(n_out, dtype=f32)            # float32 product, rounded once
    assert src.dtype == f32
    i0 = np.floor(src).astype(np.int64)
    i1 = np.minimum(i0 + 1, n_in - 1)
    l1 = src - i0.astype(f32)                                              # exact
    return torch.from_numpy(i0), torch.from_numpy(i1), torch.from_numpy(l1.astype(np.float64))


def _blend(v, ty, tx):
    (y0, y1, ly), (x0, x1, lx) = ty, tx
    lx, ly = lx[None, None, :, None], ly[None, :, None, None]
    r0, r1 = v[:, y0], v[:, y1]
    return (1 - ly) * ((1 - lx) * r0[:, :, x0] + lx * r0[:, :, x1]) + ly * ((1 - lx) * r1[:, :, x0] + lx * r1[:, :, x1])


def bilinear_ref(x, oh, ow, add=None):
    """x NHWC [B, H, W, C] -> (ref, mag) [B, oh, ow, C]; add NHWC [B, oh, ow, >= C].  mag = sum_i w_i |x_i| (+ |add|)"""
    xd = _d(x)
    B, H, W, C = xd.shape
    ty, tx = ac_taps(H, oh), ac_taps(W, ow)
    ref, mag = _blend(xd, ty, tx), _blend(xd.abs(), ty, tx)
    if add is not None:
        a = _d(add)[..., :C]
        ref, mag = ref + a, mag + a.abs()
    return ref, mag


def resize_concat_ref(xs, oh, ow):
    parts = [bilinear_ref(x, oh, ow) for x in xs]
    return torch.cat([p[0] for p in parts], -1), torch.cat([p[1] for p in parts], -1)


def bilinear_plane_ref(x, oh, ow):
    """x [H, W] -> (ref, mag) [oh, ow]"""
    ref, mag = bilinear_ref(x[None, :, :, None], oh, ow)
    return ref[0, :, :, 0], mag[0, :, :, 0]


def crop_resize_ref(img, boxes, oh, ow):
    """img [C, H, W]; boxes [P, 4] integer (x0, y0, x1, y1), x1 / y1 exclusive: the crop img[:, y0:y1, x0:x1] resized to oh x ow
    (crop_resize_planar_kernel, fake_ops.crop_resize) -> (ref, mag) [P, C, oh, ow]"""
    out = [bilinear_ref(img[:, y0:y1, x0:x1].permute(1, 2, 0)[None], oh, ow) for x0, y0, x1, y1 in boxes.tolist()]
    return torch.cat([o[0] for o in out]).permute(0, 3, 1, 2), torch.cat([o[1] for o in out]).permute(0, 3, 1, 2)


# ---------------- nearest resize ----------------
def nearest_index(n_in, n_out):
    """F.interpolate(mode='nearest'): min(floor(fl(dst * fl(in / out))), in - 1) in float32"""
    s = f32(n_in) / f32(n_out)
    v = np.arange(n_out, dtype=f32) * s
    assert v.dtype == f32
    return torch.from_numpy(np.minimum(np.floor(v).astype(np.int64), n_in - 1))


def nearest_ref(x, oh, ow):
    """x [H, W] -> [oh, ow], the selected source elements (the output must equal them bit for bit)"""
    return x.detach().cpu()[nearest_index(x.shape[0], oh)][:, nearest_index(x.shape[1], ow)]


# ---------------- roi_align (torchvision, aligned=True, sampling_ratio=-1) ----------------
def _roi_axis(start, bin_, n_out, g, i, size):
    """sample coordinate i of g along one axis for the n_out bins (float32, torchvision's order) -> valid, low, high (numpy), l (float64)"""
    c = (start + np.arange(n_out, dtype=f32) * bin_) + (f32(i + 0.5) * bin_) / f32(g)
    assert c.dtype == f32
    valid = (c >= -1.0) & (c <= size)
    c = np.maximum(c, f32(0))
    lo = np.floor(c).astype(np.int64)
    top = lo >= size - 1
    lo = np.where(top, size - 1, lo)
    hi = np.where(top, lo, lo + 1)
    c = np.where(top, lo.astype(f32), c)
    l = (c - lo.astype(f32)).astype(np.float64)                             # exact
    return torch.from_numpy(valid), torch.from_numpy(lo), torch.from_numpy(hi), torch.from_numpy(l)


def roi_align_ref(feat, rois, oh, ow, spatial_scale):
    """feat NHWC [Bf, H, W, C]; rois [K, 5] (batch, x1, y1, x2, y2) -> (ref, mag) [K, oh, ow, C].  An independent loop (oracle/third_party.py's
    roi_align computes in float32): coordinates in float32, weights and sums in float64.  mag = sum_i w_i |x_i| / count"""
    fd = _d(feat)
    Bf, H, W, C = fd.shape
    r = rois.detach().cpu().numpy().astype(f32)
    s = f32(spatial_scale)
    K = r.shape[0]
    ref = torch.zeros(K, oh, ow, C, dtype=torch.float64)
    mag = torch.zeros_like(ref)
    for k in range(K):
        fb = fd[int(r[k, 0])]
        sw, sh, ew, eh = (r[k, j] * s - f32(0.5) for j in (1, 2, 3, 4))
        roi_w, roi_h = ew - sw, eh - sh
        bin_h, bin_w = roi_h / f32(oh), roi_w / f32(ow)
        gh, gw = int(math.ceil(bin_h)), int(math.ceil(bin_w))
        count = max(gh * gw, 1)
        for iy in range(gh):
            vy, yl, yh, ly = _roi_axis(sh, bin_h, oh, gh, iy, H)
            for ix in range(gw):
                vx, xl, xh, lx = _roi_axis(sw, bin_w, ow, gw, ix, W)
                ok = (vy[:, None] & vx[None, :]).double()[..., None]
                ly_, lx_ = ly[:, None, None], lx[None, :, None]
                for (yy, wy) in ((yl, 1 - ly_), (yh, ly_)):
                    for (xx, wx) in ((xl, 1 - lx_), (xh, lx_)):
                        v = fb[yy][:, xx]                                    # [oh, ow, C]
                        ref[k] += ok * wy * wx * v
                        mag[k] += ok * wy * wx * v.abs()
        ref[k] /= count
        mag[k] /= count
    return ref, mag


def roi_align_depth_ref(feat, rois, oh, ow, spatial_scale):
    """planar feat [Bf, 1, H, W] -> (ref, mag) [K, 1, oh, ow]"""
    ref, mag = roi_align_ref(feat.permute(0, 2, 3, 1), rois, oh, ow, spatial_scale)
    return ref.permute(0, 3, 1, 2), mag.permute(0, 3, 1, 2)


# ---------------- maxpool2 ----------------
def maxpool2_ref(x):
    """x NHWC [B, H, W, C] -> [B, H // 2, W // 2, C] in x's dtype (exact; an odd last row / column is dropped)"""
    x = x.detach().cpu()
    B, H, W, C = x.shape
    v = x[:, :H // 2 * 2, :W // 2 * 2].reshape(B, H // 2, 2, W // 2, 2, C)
    return v.amax(dim=(2, 4))


# ---------------- stitch ----------------
def stitch_init_ref(pred, count, depth, mask, yx):
    """pred / count [MH, MW] as they were (NaN where never written); depth [P, ph, pw], mask [ph, pw], yx [P, 2] -> (pred, mag), count (float64)"""
    p, c = _d(pred).clone(), _d(count).clone()
    pm = torch.zeros_like(p)
    dd, m = _d(depth), _d(mask)
    P, ph, pw = dd.shape
    for i, (y0, x0) in enumerate(yx.tolist()):
        p[y0:y0 + ph, x0:x0 + pw] = dd[i] * m
        pm[y0:y0 + ph, x0:x0 + pw] = (dd[i] * m).abs()
        c[y0:y0 + ph, x0:x0 + pw] = m
    return (p, pm), c


def stitch_finish_ref(pred, count):
    r = _d(pred) / _d(count)
    return r, r.abs()


def stitch_update_ref(avg, count, depth, mask, y0, x0):
    """-> (avg', mag), (count', mag) [MH, MW]; outside the patch ref = the old value and mag = 0 (those elements must not change at all).
    mag = (|d m| + |c a|) / (c + m) for the average, c + m for the count.  A depth of another size than the mask is resized by the nearest rule."""
    a, c, m = _d(avg).clone(), _d(count).clone(), _d(mask)
    ph, pw = m.shape
    d = _d(depth) if tuple(depth.shape) == (ph, pw) else nearest_ref(depth, ph, pw).double()
    am, cm = torch.zeros_like(a), torch.zeros_like(c)
    sl = (slice(y0, y0 + ph), slice(x0, x0 + pw))
    a0, c0 = a[sl].clone(), c[sl].clone()
    a[sl] = (d * m + c0 * a0) / (c0 + m)
    am[sl] = ((d * m).abs() + (c0 * a0).abs()) / (c0 + m)
    c[sl] = c0 + m
    cm[sl] = c0 + m
    return (a, am), (c, cm)


# ---------------- Swin (G2L) ----------------
def _pad12(n):
    return (n + WIN - 1) // WIN * WIN


def _partition(v, shift):
    """[B, Hp, Wp, C] -> roll by -shift, windows of 12 x 12 -> [B nWy nWx 144, C]"""
    B, Hp, Wp, C = v.shape
    if shift > 0:
        v = torch.roll(v, shifts=(-shift, -shift), dims=(1, 2))
    return v.view(B, Hp // WIN, WIN, Wp // WIN, WIN, C).permute(0, 1, 3, 2, 4, 5).reshape(-1, C)


def swin_ln_partition_ref(x, g, b, eps, shift):
    """x NHWC [B, H, W, C] -> (ref, mag) [B Hp Wp, C]: LayerNorm over C, zero padding to multiples of 12 (after the norm), roll, partition.
    mag = (|x - mu| + |mu|) / sqrt(var + eps) |gamma| + |beta| (tests/test_float32_grade_gpu.py test_layernorm_planes_against_float64);
    padded tokens: ref = mag = 0 (they must be exactly zero)"""
    xd, gd, bd = _d(x), _d(g), _d(b)
    B, H, W, C = xd.shape
    mu, var = xd.mean(-1, keepdim=True), xd.var(-1, unbiased=False, keepdim=True)
    rstd = 1.0 / (var + float(f32(eps))).sqrt()
    ref = (xd - mu) * rstd * gd + bd
    mag = ((xd - mu).abs() + mu.abs()) * rstd * gd.abs() + bd.abs()
    pad = (0, 0, 0, _pad12(W) - W, 0, _pad12(H) - H)
    return _partition(torch.nn.functional.pad(ref, pad), shift), _partition(torch.nn.functional.pad(mag, pad), shift)


def relative_position_index():
    """[144, 144]: (yi - yj + 11) * 23 + xi - xj + 11"""
    ys, xs = torch.meshgrid(torch.arange(WIN), torch.arange(WIN), indexing="ij")
    ys, xs = ys.flatten(), xs.flatten()
    return (ys[:, None] - ys[None, :] + WIN - 1) * (2 * WIN - 1) + xs[:, None] - xs[None, :] + WIN - 1


def swin_window_attention_ref(qkv, bias_table, B, Hp, Wp, C, heads, shift, use_bias=True, use_mask=True):
    """qkv [nW 144, 3 C], bias_table [529, heads] -> (ref, mag) [nW 144, C]: softmax(q k^T / sqrt(hd) + bias + shift mask) v per window and head,
    the mask from oracle.pf_oracle.swin_shift_mask.  mag = sum_j p_j |v_j|.  use_bias / use_mask = False: the same without that term (the GPU test
    asserts that the output is far from those)"""
    from oracle.pf_oracle import swin_shift_mask
    nW, hd = qkv.shape[0] // 144, C // heads
    q, k, v = _d(qkv).view(nW, 144, 3, heads, hd).permute(2, 0, 3, 1, 4)
    attn = (q * hd ** -0.5) @ k.transpose(-2, -1)                               # [nW, heads, 144, 144]
    if use_bias:
        attn = attn + _d(bias_table)[relative_position_index().view(-1)].view(144, 144, heads).permute(2, 0, 1)[None]
    if shift > 0 and use_mask:
        mask = swin_shift_mask(Hp, Wp, WIN, shift, "cpu").double()              # [nW / B, 144, 144]
        attn = (attn.view(B, nW // B, heads, 144, 144) + mask[None, :, None]).view(nW, heads, 144, 144)
    p = attn.softmax(-1)
    back = lambda t: t.transpose(1, 2).reshape(nW * 144, C)
    return back(p @ v), back(p @ v.abs())


def swin_unpartition_add_ref(proj, shortcut, shift):
    """proj [B nW 144, C] (windows of the padded, rolled map), shortcut NHWC [B, H, W, C] -> (ref, mag) [B, H, W, C]; mag = |shortcut| + |proj|"""
    s = _d(shortcut)
    B, H, W, C = s.shape
    Hp, Wp = _pad12(H), _pad12(W)
    v = _d(proj).view(B, Hp // WIN, Wp // WIN, WIN, WIN, C).permute(0, 1, 3, 2, 4, 5).reshape(B, Hp, Wp, C)
    if shift > 0:
        v = torch.roll(v, shifts=(shift, shift), dims=(1, 2))
    v = v[:, :H, :W]
    return s + v, s.abs() + v.abs()


# ---------------- metric-bins head ----------------
def attractor_ref(A, n_attr, b_prev, h, w, a_stride=1, a_eps=0.0, attractor_type="inv", kind="mean"):
    """A [B, h, w, >= (n_attr - 1) a_stride + 1], b_prev [B, hp, wp, nb] -> (ref, mag) [B, h, w, nb]:  c = up(b_prev), a_i = A[i a_stride] + a_eps,
    d_i = dx / (1 + 300 dx^2) ('inv') or exp(-300 dx^2) dx ('exp') with dx = a_i - c, out = c + scale sum_i d_i, scale = 1 / n_attr ('mean') or 1.
    mag = |c| + scale sum_i |d_i|"""
    c, _ = bilinear_ref(b_prev, h, w)
    a = _d(A)[..., :(n_attr - 1) * a_stride + 1:a_stride] + float(f32(a_eps))   # [B, h, w, n_attr]
    dx = a[..., :, None] - c[..., None, :]                                       # [B, h, w, n_attr, nb]
    d = torch.exp(-300.0 * dx * dx) * dx if attractor_type == "exp" else dx / (1 + 300.0 * dx * dx)
    scale = 1.0 / n_attr if kind == "mean" else 1.0
    return c + scale * d.sum(-2), c.abs() + scale * d.abs().sum(-2)


def logbinom_logc(nb):
    """log C(n, k) in the Stirling form of the log-binomial head, k = 0 .. nb - 1: the arguments n + eps, k + eps, n - k + eps (eps = 1e-7) are the
    float32 values the float32 definition forms (63 + 1e-7 = 63, k + 1e-7 = k for k >= 1), the logarithms and products float64"""
    eps = f32(1e-7)
    n_ = f32(nb - 1) + eps
    k_ = np.arange(nb, dtype=f32) + eps
    inner = (n_ - k_) + eps
    assert k_.dtype == f32 and inner.dtype == f32
    n_, k_, inner = float(n_), torch.from_numpy(k_.astype(np.float64)), torch.from_numpy(inner.astype(np.float64))
    return n_ * math.log(n_) - k_ * torch.log(k_) - (n_ - k_) * torch.log(inner)


def logbinom_depth_ref(pt, centers, h, w, min_temp, max_temp):
    """pt [B, h, w, >= 4] (p0, p1, t0, t1, softplus applied), centers [B, hc, wc, nb] -> (ref, mag) [B, h, w]:
    p = p0 / (p0 + p1), t = (max_temp - min_temp) t0 / (t0 + t1) + min_temp (each + 1e-4 first), softmax_k((log C(n, k) + k log p + (n - k) log(1 - p)) / t)
    . up(centers).  mag = sum_k p_k |center_k|.  A float64 pt is taken as it is (bins_tail_ref hands over the unrounded softplus outputs)"""
    e4 = float(f32(1e-4))
    q = _d(pt)[..., :4] + e4
    p = q[..., 0] / (q[..., 0] + q[..., 1])
    t = q[..., 2] / (q[..., 2] + q[..., 3])
    lo, hi = float(f32(min_temp)), float(f32(max_temp))
    t = ((hi - lo) * t + lo)[..., None]
    om = torch.clamp(1 - p, e4, 1.0)[..., None]
    p = torch.clamp(p, e4, 1.0)[..., None]
    nb = centers.shape[-1]
    k = torch.arange(nb, dtype=torch.float64)
    yk = (logbinom_logc(nb) + k * torch.log(p) + (nb - 1 - k) * torch.log(om)) / t
    pr = yk.softmax(-1)
    c, cm = bilinear_ref(centers, h, w)
    return (pr * c).sum(-1), (pr * cm).sum(-1)


def bins_tail_ref(last, rel, emb, w0, b0, w2, b2, centers, H, W, min_temp, max_temp):
    """the fused metric-bins tail (csrc/imageops.hip bins_tail_kernel) in float64 from its float32 operands: last [B, H, W, 32], rel [B, H, W, 8] or
    None, emb [B, he, we, 128], w0 [80, ctot] over the channel order of the CLB buffer (last, embedding, rel), b0 [80], w2 [4, 80], b2 [4], centers
    [B, hc, wc, 64] -> (depth, mag) [B, H, W].  x = cat[last, up(emb), rel] (bilinear_ref: the float32 source coordinate, float64 blend), W0 x + b0,
    erf-GELU, W2 h + b2, softplus (the true log(1 + e^v): the float32 definition's switch to v above 20 moves a value by e^-20 = 2e-9), then
    logbinom_depth_ref on the UNROUNDED pt: nothing between the operands and the depth is rounded to float32.  mag = sum_k p_k |c_k|."""
    e, _ = bilinear_ref(emb, H, W)
    x = torch.cat([_d(last), e] + ([] if rel is None else [_d(rel)]), -1)
    h = x @ _d(w0).t() + _d(b0)
    h = 0.5 * h * (1 + torch.erf(h * math.sqrt(0.5)))
    pt = h @ _d(w2).t() + _d(b2)
    pt = torch.logaddexp(pt, torch.zeros_like(pt))
    return logbinom_depth_ref(pt, centers, H, W, min_temp, max_temp)


def seed_bin_centers_ref(x, n_bins, lo, hi, bounded, normalize):
    """x [..., >= n_bins] -> (ref, mag) [..., n_bins] (csrc/imageops.hip seed_bin_centers_kernel; lo, hi, 1e-3 the float32 scalars of the C ABI):
    bounded: Bn = x + 1e-3, width_k = (hi - lo) Bn_k / sum Bn, edges = lo + running sum of the widths, centre_k = (e_k + e_k+1) / 2;
    normalize: (centre - lo) / (hi - lo).  mag = the sum of the absolute values of the terms of an element: the running sums |lo| + sum |width| of the
    two edges of a centre on the bounded path (|x| otherwise), and (mag + |lo|) / (hi - lo) after the normalisation"""
    c = _d(x)[..., :n_bins]
    lo, hi = float(f32(lo)), float(f32(hi))
    mag = c.abs()
    if bounded:
        bn = c + float(f32(1e-3))
        w = (hi - lo) * (bn / bn.sum(-1, keepdim=True))
        zero = torch.zeros_like(w[..., :1])
        edges = lo + torch.cumsum(torch.cat([zero, w], -1), -1)
        emag = abs(lo) + torch.cumsum(torch.cat([zero, w.abs()], -1), -1)
        c, mag = 0.5 * (edges[..., :-1] + edges[..., 1:]), 0.5 * (emag[..., :-1] + emag[..., 1:])
    if normalize:
        c, mag = (c - lo) / (hi - lo), (mag + abs(lo)) / (hi - lo)
    return c, mag


def bounded_bin_centers_ref(b, lo, hi):
    """b [..., n_bins] -> (ref, mag): ref = clip(sort((hi - lo) b + lo), lo, hi) along the bins, mag per pixel = max over its bins of
    (hi - lo) |b| + |lo| (broadcast to the bins).  Sorting is 1-Lipschitz in the sup norm -- if |u_k - v_k| <= e for every k then
    |sort(u)_j - sort(v)_j| <= e for every j (the j-th smallest of v lies between the j-th smallest of u - e and of u + e) -- and so is clipping:
    every sorted, clipped element is within the largest error of the unsorted elements of its pixel, which k 2^-24 max_k mag_k bounds."""
    bd = _d(b)
    lo, hi = float(f32(lo)), float(f32(hi))
    ref = torch.clip(torch.sort((hi - lo) * bd + lo, dim=-1)[0], lo, hi)
    mag = ((hi - lo) * bd.abs() + abs(lo)).amax(-1, keepdim=True).expand_as(ref)
    return ref, mag


# ---------------- inputs and cases shared by the CPU and the GPU test ----------------
def features(shape, seed, dtype=torch.float32, amp=2.0 ** -16):
    """mid-range values with low-amplitude detail: a per-channel level in [0.5, 1.5] plus amp * N(0, 1) per element (channels = the last axis).
    Positive, so mag = |ref| for every interpolation; a wrong tap or weight moves an element by ~amp (1e2 float32 roundings, 1e-4 of the maximum)"""
    g = torch.Generator().manual_seed(seed)
    level = 0.5 + torch.rand(shape[-1], generator=g, dtype=torch.float64)
    return (level + amp * torch.randn(*shape, generator=g, dtype=torch.float64)).to(dtype)


# h, w -> oh, ow, C
RESIZE_CASES = [(14, 19, 28, 37, 64), (56, 74, 28, 37, 32), (8, 11, 8, 11, 64), (5, 7, 1, 1, 8), (1, 1, 6, 9, 8), (30, 3, 31, 2, 24),
                (37, 50, 9, 200, 16), (2, 4000, 3, 4100, 8)]
PLANE_CASES = [(40, 52, 96, 130), (96, 130, 40, 52)]
# boxes (x0, y0, x1, y1) on a 3 x 96 x 130 image to 28 x 42: touching the top-left, the bottom-right, the right, the bottom border, interior, and
# one the size of the output
CROP_BOXES = [[0, 0, 65, 48], [65, 48, 130, 96], [88, 7, 130, 35], [13, 60, 78, 96], [13, 7, 78, 55], [50, 30, 92, 58]]
# B, H, W, C, heads: head_dim 2, 4, 8, 16, 32
SWIN_CASES = [(1, 12, 12, 64, 32), (1, 12, 24, 64, 16), (1, 13, 24, 64, 8), (2, 17, 12, 128, 8), (1, 14, 19, 256, 8)]
ROI_FEATS = [(4, 6, 64), (28, 37, 64), (112, 154, 32)]
# inside, touching the far corner, partly outside (x1 > W), wholly outside (negative); image coordinates of a 112 x 154 map
ROIS = [[0, 0.0, 0.0, 77.0, 56.0], [0, 77.0, 56.0, 154.0, 112.0], [0, 38.5, 28.0, 115.5, 84.0], [0, 100.25, 60.5, 177.25, 116.5],
        [0, -90.0, -70.0, -13.0, -14.0]]


# ---------------- operands of the metric-bins tail, the bin centres and the copies (tests/test_f64_image_ref_cpu.py, tests/test_tail_grade_gpu.py) ----
MIN_TEMP, MAX_TEMP = 0.0212, 50.0
TAIL_KINDS = ("random", "sorted", "t_low", "t_high", "p_ends", "softplus_linear")
# B, H, W: one pixel; one partial group of 16; a tail of 4; one row; more pixel groups than the 512 x 4 the grid covers in one pass (tail of 14)
TAIL_SHAPES = [(1, 1, 1), (1, 3, 5), (2, 37, 50), (1, 1, 40), (1, 150, 221)]
TAIL_EMB_GRID, TAIL_CEN_GRID = (21, 29), (11, 15)
# name -> (emb grid, centres grid) at 2 x 37 x 50; None = the output's own size (scale exactly 1)
TAIL_GRIDS = {"emb_full_size": ((37, 50), TAIL_CEN_GRID), "emb_1x1": ((1, 1), TAIL_CEN_GRID), "cen_on_emb_grid": (TAIL_EMB_GRID, TAIL_EMB_GRID)}


def tail_operands(kind, ctot, B, H, W, emb_grid=TAIL_EMB_GRID, cen_grid=TAIL_CEN_GRID, seed=0):
    """seeded operands of the fused tail -> dict(last [B, H, W, 32], rel [B, H, W, 8] or None (ctot 160), emb [B, he, we, 128], w0 [80, ctot] over the
    CLB buffer's channel order (last, embedding, rel), b0, w2 [4, 80], b2, centers [B, hc, wc, 64]), float32.  Kinds:
      random           N(0, 1) features, weights N(0, 1 / fan-in), biases 0.1 N(0, 1); centres uniform in [0.5, 5.5), independent per position and bin, NOT sorted
      sorted           the same with the centres sorted along the bins (tests/op_checks.py bins_tail)
      t_low, t_high    b2 -+ 30 on t0 and +- 30 on t1: t0 / (t0 + t1) is 3e-6 / 1 - 3e-6, the temperature min_temp / max_temp
      p_ends           hidden channels 0 and 1 see only +-last[..., 0], which is +50 in the first half of the pixels and -50 in the second, and drive
                       (p0, p1) to (50, 0) / (0, 50): 1 - p, then p, lies below the 1e-4 clamp
      softplus_linear  b2 + (20, 20.5) on p0, p1: about half of their pre-activations above 20, where softplus is the identity"""
    assert kind in TAIL_KINDS and ctot in (160, 168)
    g = torch.Generator().manual_seed(1000 * TAIL_KINDS.index(kind) + ctot + 7 * H + W + seed)
    (he, we), (hc, wc) = emb_grid, cen_grid
    r = lambda *s: torch.randn(*s, generator=g)
    o = dict(last=r(B, H, W, 32), rel=r(B, H, W, 8) if ctot == 168 else None, emb=r(B, he, we, 128), w0=r(80, ctot) / ctot ** 0.5, b0=0.1 * r(80),
             w2=r(4, 80) / 80 ** 0.5, b2=0.1 * r(4), centers=torch.rand(B, hc, wc, 64, generator=g) * 5 + 0.5)
    if kind == "sorted":
        o["centers"] = o["centers"].sort(-1).values.contiguous()
    if kind in ("t_low", "t_high"):
        s = -30.0 if kind == "t_low" else 30.0
        o["b2"][2] += s
        o["b2"][3] -= s
    if kind == "p_ends":
        first = (torch.arange(B * H * W) < (B * H * W + 1) // 2).view(B, H, W)
        o["last"][..., 0] = torch.where(first, 50.0, -50.0)
        o["w0"][:, 0] = 0
        o["w0"][:2] = 0
        o["w0"][0, 0], o["w0"][1, 0] = 1.0, -1.0
        o["b0"][:2] = 0
        o["w2"][:, :2] = torch.tensor([[1.0, -1.0], [-1.0, 1.0], [0.0, 0.0], [0.0, 0.0]])
    if kind == "softplus_linear":
        o["b2"][0] += 20.0
        o["b2"][1] += 20.5
    return o


def tail_ref(o, H, W):
    return bins_tail_ref(o["last"], o["rel"], o["emb"], o["w0"], o["b0"], o["w2"], o["b2"], o["centers"], H, W, MIN_TEMP, MAX_TEMP)


def tail_pack(o):
    """-> packing.BinsTail of the two layers (with .mlp0 / .mlp2, the packed layers of the unfused route)"""
    from patchfusion_amd import packing as pk
    mlp0 = pk.pack_conv(o["w0"][:, :, None, None].clone(), o["b0"].clone(), dtype=torch.float32)
    mlp2 = pk.pack_conv(o["w2"][:, :, None, None].clone(), o["b2"].clone(), dtype=torch.float32)
    tw = pk.bins_tail_weights(mlp0, mlp2, 128)
    assert tw is not None and tw.nq == (11 if o["rel"] is not None else 10)
    return tw


def tail_clb(o, ld=None, off=0, device="cpu"):
    """the CLB buffer of the operands: [B, H, W, ctot] = last | NaN (the embedding slice, which the fused kernel must not read) | rel, as channels
    [off, off + ctot) of a NaN-filled buffer of ld channels (ld None: ctot, contiguous)"""
    B, H, W, _ = o["last"].shape
    ctot = o["w0"].shape[1]
    wide = torch.full((B, H, W, ld or ctot), float("nan"))
    wide[..., off:off + 32] = o["last"]
    if o["rel"] is not None:
        wide[..., off + 160:off + 168] = o["rel"]
    return wide.to(device)[..., off:off + ctot]


def seed_operands(shape, n_bins, ld, seed=23):
    """relu(N(0, 1)) [*shape, n_bins] (the SeedBinRegressor's activation output, with exact zeros) as channels [0, n_bins) of a NaN-filled [*shape, ld]"""
    wide = torch.full((*shape, ld), float("nan"))
    wide[..., :n_bins] = torch.relu(torch.randn(*shape, n_bins, generator=torch.Generator().manual_seed(seed + n_bins)))
    return wide[..., :n_bins]


def bounded_operands(npix, n_bins, seed=24):
    """[1, 1, npix, n_bins]: 0.5 + 0.6 N(0, 1) (a fifth outside [0, 1], unsorted); the first min(4, npix / 2) pixels rounded to integers (ties, and
    values outside [0, 1]); +0 and -0 in the first pixel, one bin set to the largest of its pixel in the second (a tie at the top)"""
    b = 0.5 + 0.6 * torch.randn(1, 1, npix, n_bins, generator=torch.Generator().manual_seed(seed + n_bins + npix))
    b[0, 0, :min(4, npix // 2)] = b[0, 0, :min(4, npix // 2)].round()
    b[0, 0, 0, 0], b[0, 0, 0, -1] = 0.0, -0.0
    if npix > 1:
        b[0, 0, 1, 0] = b[0, 0, 1].max()
    return b


def bf16_edge_values():
    """float32 values whose rounding to bfloat16 separates round-to-nearest-even from truncation and from round-half-up: exact ties above an even and
    above an odd bfloat16 (both signs), the float32 neighbours of a tie, a tie at the top of a binade and the largest float32 below 2 (both round up
    into the next binade)"""
    bits = [0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000, 0x3F807FFF, 0x3F808001, 0x3FFF8000, 0x3FFFFFFF]
    return torch.tensor(bits, dtype=torch.int64).to(torch.int32).view(torch.float32)


def copy_operands(shape, dt, seed=31):
    """N(0, 1) [*shape] of dtype dt; a float32 tensor carries bf16_edge_values() in its first and its last elements"""
    x = torch.randn(*shape, generator=torch.Generator().manual_seed(seed + shape[-1]))
    if dt == torch.float32:
        e = bf16_edge_values()
        x.view(-1)[:e.numel()] = e
        x.view(-1)[-e.numel():] = e
    return x.to(dt)


def _tail_cases():
    """(name, kind, ctot, (B, H, W), emb grid, centres grid): every shape with random operands, every kind and every extra grid at 2 x 37 x 50; both
    channel counts throughout"""
    cases = []
    for ctot in (168, 160):
        for shp in TAIL_SHAPES:
            cases.append((f"random_c{ctot}_{'x'.join(map(str, shp))}", "random", ctot, shp, TAIL_EMB_GRID, TAIL_CEN_GRID))
        for kind in TAIL_KINDS[1:]:
            cases.append((f"{kind}_c{ctot}_2x37x50", kind, ctot, (2, 37, 50), TAIL_EMB_GRID, TAIL_CEN_GRID))
        for name, (eg, cg) in TAIL_GRIDS.items():
            cases.append((f"{name}_c{ctot}_2x37x50", "random", ctot, (2, 37, 50), eg, cg))
    return cases


TAIL_CASES = _tail_cases()
# lo, hi of the counted bin-centre checks: hi - lo is a float32 number, so the two roundings counted (the product and the sum, or the difference and
# the quotient) are all there are; at the head's own 1e-3, 80 the float32 difference 79.999 is itself rounded (0.8 * 2^-24), a third rounding that an
# unfused float32 evaluation adds to its two
EXACT_RANGES = [(2.0 ** -10, 80.0), (-2.5, 10.0)]
K_BOUNDED, K_SEED_NORM = 2, 2
