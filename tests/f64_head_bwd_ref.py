"""Float64 references, per-element magnitudes, float32 restatements, cases and bars of the head's backward kernels (csrc/head_bwd.hip):
pf_conv1x1_wgrad, pf_resize_bilinear_bwd, pf_attractor_bwd, pf_logbinom_depth_bwd, pf_act_bwd, pf_silog_loss_bwd.  Style and metric of
tests/f64_image_ref.py / tests/f64_eval_ref.py; used by tests/test_head_bwd_grade_gpu.py, checked on the CPU by tests/test_f64_head_bwd_ref_cpu.py.
No GPU needed.

Every *_ref function takes the float32 operands the kernel sees and returns (ref, mag) in float64 for EVERY output element.  What the operation
defines in float32 is float32 here too (the rule of f64_image_ref.py): the source coordinates of a resize (f64_image_ref.ac_taps), the constants
1e-4f and 1e-7f, added in float32, the Stirling table of the log-binomial (the float32 torch expression of hip_ops._logbinom_logc) and every scalar
of the C ABI (min_temp = 0.0212 is 3e-8 from its float32 value, and y / t multiplies that).  Everything else is float64.

mag is the sum of the absolute values of the terms of an element; where a term is a function of a rounded difference its first-order sensitivity
to the operands of that difference is added (attractor: f'' (|A| + mag_c); log-binomial: the exponent's e_k; softplus: y e^-y).

The log-binomial is evaluated RELATIVE TO THE PEAK BIN r (arg-max of y_k / t, ties to the highest bin), like the kernel:
    y_k - y_r = (logc_k - logc_r) + (k - r) (log x - log(1 - x)),   c_k - c_r,   s_k = sum dz_k (k - r),   s_nk = -s_k,   s_y = sum dz_k (y_k - y_r)
(sum_k dz_k = 0, so any reference bin gives the same value).  The full-size form of tests/head_bwd_ref.logbinom_bwd rounds c_k - depth and
sum dz_k k at the size of the centres and of y / t: where the softmax is one-hot its float64 error (2^-53 x 32 x 63 / t) exceeds the element and
the sign comes out wrong (tests/test_f64_head_bwd_ref_cpu.py records the pixel against mpmath); that function is a norm-wise truth only.

The *_f32 functions restate each kernel's arithmetic in numpy float32, operation by operation (sums in numpy's order): the evidence, before any GPU
run, that the bars can be met.  The *_torch functions are the baselines: torch float32 autograd through oracle/pf_oracle.py's lines on a device."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from tests.f64_image_ref import (FLOOR, K_BILERP, U, ac_scale, ac_taps, baseline_bar, bilinear_ref, counted_bar)     # noqa: F401
from tests.f64_ref import TINY, decade_spread, errors                                                                # noqa: F401

f32 = np.float32
F64 = torch.float64
E4, E7 = f32(1e-4), f32(1e-7)
MIN_TEMP, MAX_TEMP = 0.0212, 50.0
LO, HI = float(f32(1e-3)), 80.0                  # (min_depth, max_depth) as the float32 numbers the C ABI passes

# grid_for of csrc/head_bwd.hip caps a grid at 16 384 blocks: the element kernels (256 threads, one element each) cover 16384 x 256 elements in one
# pass, the pixel kernels (256 threads = 4 waves, one wave per pixel) 16384 x 4 pixels; past that the grid-stride loops run
GRID_CAP = 16384
ELEM_CAPACITY = GRID_CAP * 256
PIXEL_CAPACITY = GRID_CAP * 4

# roundings counted on the longest path of the log-binomial kernel (derivation: tests/test_head_bwd_grade_gpu.py)
K_LB_DCUP, K_LB_DPT = 15, 55


def _d(t):
    return t.detach().cpu().double()


def _np32(t):
    return t.detach().cpu().numpy().astype(f32)


# ---------------- weight gradient ----------------
def wgrad_ref(dy, x):
    """dy [P, N], x [P, K] -> ((dW, mag) [N, K], (db, mag) [N]): dW = sum_p dy x, mag = sum_p |dy| |x|; db = sum_p dy, mag = sum_p |dy|"""
    d, xx = _d(dy), _d(x)
    return (d.t() @ xx, d.abs().t() @ xx.abs()), (d.sum(0), d.abs().sum(0))


def wgrad_f32(dy, x, rows=0, drop_pixel=None, k_tail_from=None):
    """float32 restatement: partial sums over splits of `rows` pixels (0: one split), pixel after pixel, then the splits added in order.
    Planted defects: drop_pixel = j leaves pixel j of every split out; k_tail_from = a [P] column (a pad column of the strided operand) read in
    place of x's last column"""
    d, xx = _np32(dy), _np32(x).copy()
    if k_tail_from is not None:
        xx[:, -1] = _np32(k_tail_from)
    P = d.shape[0]
    rows = rows or P
    dw, db = np.zeros((d.shape[1], xx.shape[1]), f32), np.zeros(d.shape[1], f32)
    for s in range(0, P, rows):
        pw, pb = np.zeros_like(dw), np.zeros_like(db)
        for p in range(s, min(s + rows, P)):
            if drop_pixel is not None and p - s == drop_pixel:
                continue
            pw += np.outer(d[p], xx[p])
            pb += d[p]
        dw, db = dw + pw, db + pb
    return torch.from_numpy(dw), torch.from_numpy(db)


def wgrad_torch(dy, x):
    return torch.matmul(dy.t(), x), dy.sum(0)


# ---------------- resize adjoint ----------------
def tap_matrix(n_in, n_out, dtype=np.float64, f64_coords=False, short_high=False):
    """[n_out, n_in] interpolation matrix of one axis from the forward's float32 coordinates (ac_taps); in float32 l0 = fl(1 - l1) as the kernel
    forms it.  Planted defects: f64_coords takes src = d (n_in - 1) / (n_out - 1) in float64; short_high drops, for every source index, the last
    destination that touches it (a destination range one short on the high side)"""
    i0, i1, l1 = (t.numpy() for t in ac_taps(n_in, n_out))
    if f64_coords:
        src = (n_in - 1) / (n_out - 1) * np.arange(n_out) if n_out > 1 else np.zeros(n_out)
        i0 = np.minimum(np.floor(src).astype(np.int64), n_in - 1)
        i1 = np.minimum(i0 + 1, n_in - 1)
        l1 = src - i0
    M = np.zeros((n_out, n_in), dtype)
    l1 = l1.astype(dtype)
    np.add.at(M, (np.arange(n_out), i0), dtype(1) - l1)
    np.add.at(M, (np.arange(n_out), i1), l1)
    if short_high:
        for s in range(n_in):
            nz = np.nonzero(M[:, s])[0]
            if len(nz) > 1:
                M[nz[-1], s] = 0
    return M


def resize_bwd_ref(dy, H, W, init=None):
    """dy [B, OH, OW, C] -> (ref, mag) [B, H, W, C]: M_y^T dy M_x and the same with |dy|; init (accumulate) adds init and |init|.  mag == 0: no
    destination touches the element, which must come back exactly 0.0 (exactly init under accumulate)"""
    d = _d(dy)
    My, Mx = torch.from_numpy(tap_matrix(H, d.shape[1])), torch.from_numpy(tap_matrix(W, d.shape[2]))
    ref, mag = torch.einsum("oh,pw,bopc->bhwc", My, Mx, d), torch.einsum("oh,pw,bopc->bhwc", My, Mx, d.abs())
    if init is not None:
        ref, mag = ref + _d(init), mag + _d(init).abs()
    return ref, mag


def resize_bwd_f32(dy, H, W, init=None, **defect):
    d = _np32(dy)
    My, Mx = tap_matrix(H, d.shape[1], f32, **defect), tap_matrix(W, d.shape[2], f32, **defect)
    r = np.einsum("pw,bopc->bowc", Mx, d).astype(f32)
    s = np.einsum("oh,bowc->bhwc", My, r).astype(f32)
    if init is not None:
        s = _np32(init) + s
    return torch.from_numpy(s)


def resize_bwd_torch(dy, H, W, init=None):
    """autograd through pf_oracle.up (F.interpolate, align_corners=True) in float32 on dy's device"""
    from oracle import pf_oracle
    B, OH, OW, C = dy.shape
    x = torch.zeros(B, C, H, W, device=dy.device, requires_grad=True)
    pf_oracle.up(x, (OH, OW)).backward(dy.permute(0, 3, 1, 2))
    g = x.grad.permute(0, 2, 3, 1)
    return g if init is None else init + g


# ---------------- attractor ----------------
def _fp_fpp(dx, at):
    """f'(dx) and f''(dx) of f = dx / (1 + 300 dx^2) ('inv') or exp(-300 dx^2) dx ('exp'), q = 300 dx^2"""
    q = 300.0 * dx * dx
    if at == "exp":
        e = torch.exp(-q)
        return e * (1 - 2 * q), 600.0 * dx * e * (2 * q - 3)
    return (1 - q) / (1 + q) ** 2, 600.0 * dx * (q - 3) / (1 + q) ** 3


def attractor_bwd_ref(A, b_prev, g, at, kind):
    """A [B,h,w,n_attr], b_prev [B,hp,wp,nb], g [B,h,w,nb] -> ((dA, mag) [B,h,w,n_attr], (d_b_c, mag) [B,h,w,nb]):
    c = up(b_prev) (float32 coordinates), dx = A_i - c_j, dA_i = s sum_j g_j f'(dx), dc_j = g_j (1 - s sum_i f'(dx)).  dx is a rounded
    difference of operands of size |A_i| and mag_c_j (the blend of |b_prev|), so f' carries |f''| (|A_i| + mag_c_j)"""
    a, gd = _d(A), _d(g)
    c, mc = bilinear_ref(b_prev, a.shape[1], a.shape[2])
    s = 1.0 / a.shape[-1] if kind == "mean" else 1.0
    fp, fpp = _fp_fpp(a[..., :, None] - c[..., None, :], at)                        # [B,h,w,i,j]
    mfp = fp.abs() + fpp.abs() * (a.abs()[..., :, None] + mc[..., None, :])
    dA, mA = s * (fp * gd[..., None, :]).sum(-1), s * (mfp * gd.abs()[..., None, :]).sum(-1)
    return (dA, mA), (gd * (1 - s * fp.sum(-2)), gd.abs() * (1 + s * mfp.sum(-2)))


def bilerp_f32(v, oh, ow):
    """the kernels' float32 blend ly.l0 (lx.l0 v00 + lx.l1 v01) + ly.l1 (lx.l0 v10 + lx.l1 v11), l0 = fl(1 - l1); v numpy [B,H,W,C]"""
    (y0, y1, ly), (x0, x1, lx) = ac_taps(v.shape[1], oh), ac_taps(v.shape[2], ow)
    ly1, lx1 = ly.numpy().astype(f32)[None, :, None, None], lx.numpy().astype(f32)[None, None, :, None]
    ly0, lx0 = f32(1) - ly1, f32(1) - lx1
    r0, r1 = v[:, y0.numpy()], v[:, y1.numpy()]
    x0, x1 = x0.numpy(), x1.numpy()
    out = ly0 * (lx0 * r0[:, :, x0] + lx1 * r0[:, :, x1]) + ly1 * (lx0 * r1[:, :, x0] + lx1 * r1[:, :, x1])
    assert out.dtype == f32
    return out


def attractor_bwd_f32(A, b_prev, g, at, kind, drop_bins_from=None, no_scale=False):
    """Planted defects: drop_bins_from = j0 leaves the bins from j0 out of dA's sum and writes no d_b_c there (it stays 0); no_scale forgets
    `scale` on 'mean'"""
    a, gg = _np32(A), _np32(g)
    c = bilerp_f32(_np32(b_prev), a.shape[1], a.shape[2])
    s = f32(1.0) if kind == "sum" or no_scale else f32(1.0) / f32(a.shape[-1])
    dx = a[..., :, None] - c[..., None, :]
    q = f32(300.0) * (dx * dx)
    fp = np.exp(-q) * (f32(1) - f32(2) * q) if at == "exp" else (f32(1) - q) / ((f32(1) + q) * (f32(1) + q))
    assert fp.dtype == f32
    live = np.ones(c.shape[-1], bool)
    if drop_bins_from is not None:
        live[drop_bins_from:] = False
    dA = s * (gg[..., None, :] * fp)[..., live].sum(-1, dtype=f32)
    dc = np.where(live, gg * (f32(1) - s * fp.sum(-2, dtype=f32)), f32(0))
    return torch.from_numpy(dA.astype(f32)), torch.from_numpy(dc.astype(f32))


def attractor_bwd_torch(A, b_prev, g, at, kind):
    """autograd through the oracle's float32 lines (pf_oracle.up, pf_oracle._attractor_delta) on A's device -> (dA, d_b_c) NHWC"""
    from oracle import pf_oracle
    nchw = lambda t: t.permute(0, 3, 1, 2).contiguous()
    a = nchw(A).requires_grad_(True)
    c = pf_oracle.up(nchw(b_prev), A.shape[1:3]).requires_grad_(True)
    (c + pf_oracle._attractor_delta(a, c, dict(attractor_type=at, attractor_kind=kind))).backward(nchw(g))
    return a.grad.permute(0, 2, 3, 1), c.grad.permute(0, 2, 3, 1)


# ---------------- log-binomial ----------------
def logc_table(nb):
    """log C(nb - 1, k) in the Stirling form, float32 torch arithmetic: the expression of hip_ops._logbinom_logc (the GPU test asserts equality)"""
    eps = 1e-7
    k = torch.arange(nb, dtype=torch.float32) + eps
    n = torch.full((1,), float(nb - 1)) + eps
    return n * torch.log(n) - k * torch.log(k) - (n - k) * torch.log(n - k + eps)


ORDINARY, X_CLAMP, OM_CLAMP, COLD = 0, 1, 2, 3
CLASS_NAMES = {ORDINARY: "ordinary", X_CLAMP: "x_clamp", OM_CLAMP: "om_clamp", COLD: "cold"}
COLD_BELOW = 0.5                                 # temperature under which a pixel counts as cold (logbinom_case's own start at 0.6)


def _lb_front(pt, min_temp, max_temp):
    """the float32-defined head of the log-binomial in float64: p_i = fl32(pt_i + 1e-4f); prob, t, 1 - prob, the clamped values, their logs"""
    q = torch.from_numpy((_np32(pt)[..., :4] + E4).astype(np.float64))
    p0, p1, t0, t1 = q.unbind(-1)
    lo, hi = float(f32(min_temp)), float(f32(max_temp))
    prob, t = p0 / (p0 + p1), (hi - lo) * (t0 / (t0 + t1)) + lo
    om_raw = 1 - prob
    xc, om = prob.clamp(float(E4), 1.0), om_raw.clamp(float(E4), 1.0)
    inx, inom = (prob >= float(E4)) & (prob <= 1.0), (om_raw >= float(E4)) & (om_raw <= 1.0)
    return p0, p1, t0, t1, prob, t, om_raw, xc, om, inx, inom, hi - lo


def logbinom_bwd_ref(pt, centers, gd, min_temp=MIN_TEMP, max_temp=MAX_TEMP):
    """pt [B,h,w,>=4], centers [B,hc,wc,nb], gd [B,h,w] -> dict(d_pt=(ref, mag) [B,h,w,4], d_cup=(ref, mag) [B,h,w,nb], cls [B,h,w] (class of
    the pixel), r [B,h,w] (the peak bin), probs, depth_rel).  Peak-relative form (module docstring); magnitudes:
        e_k          = (|logc_k - logc_r| + |k - r| (|log x| + |log(1 - x)| + [1 - x unclamped] x / (1 - x))) / t
                       (the last term: log(1 - x) is a function of the rounded difference 1 - x, first-order sensitivity to x)
        mag_probs_k  = probs_k (1 + e_k + sum_m probs_m e_m) + 2^-102     (the floor: a float32 expf may flush below 2^-126)
        mag_dcup     = |g| mag_probs
        mag(c_k - depth) = |c_k - c_r| + sum_m probs_m |c_m - c_r| + mag_c_k + mag_c_r
        mag_dz_k     = |g| (mag_probs_k |c_k - depth| + probs_k mag(c_k - depth))
        mag_s_k      = sum_k mag_dz_k |k - r|,   mag_s_y = sum_k (mag_dz_k |y_k - y_r| + |dz_k| e_k t)
    and the clamps and the two quotient rules carried through as absolute values"""
    p0, p1, t0, t1, prob, t, om_raw, xc, om, inx, inom, span = _lb_front(pt, min_temp, max_temp)
    nb = centers.shape[-1]
    B, h, w = prob.shape
    logc = logc_table(nb).double()
    k = torch.arange(nb, dtype=F64)
    lp, lq = torch.log(xc), torch.log(om)
    z = (logc + k * lp[..., None] + (nb - 1 - k) * lq[..., None]) / t[..., None]
    r = (nb - 1) - z.flip(-1).argmax(-1)                                            # ties: the highest bin
    kr, lcr = (k - r[..., None].double()), logc[r][..., None]
    dy = (logc - lcr) + kr * (lp - lq)[..., None]
    sens = torch.where(inom, prob / om_raw.clamp_min(1e-300), torch.zeros_like(prob))
    e = ((logc - lcr).abs() + kr.abs() * (lp.abs() + lq.abs() + sens)[..., None]) / t[..., None]
    probs = torch.softmax(dy / t[..., None], -1)
    c, mc = bilinear_ref(centers, h, w)
    cr, mcr = c.gather(-1, r[..., None]), mc.gather(-1, r[..., None])
    dc = c - cr
    depth_rel = (probs * dc).sum(-1, keepdim=True)
    cmd = dc - depth_rel
    g = _d(gd)[..., None]
    dz = probs * cmd * g
    s_k, s_y = (dz * kr).sum(-1), (dz * dy).sum(-1)
    m_probs = probs * (1 + e + (probs * e).sum(-1, keepdim=True)) + 2.0 ** -102
    m_cmd = dc.abs() + (probs * dc.abs()).sum(-1, keepdim=True) + mc + mcr
    m_dz = g.abs() * (m_probs * cmd.abs() + probs * m_cmd)
    m_sk = (m_dz * kr.abs()).sum(-1)
    m_sy = (m_dz * dy.abs() + dz.abs() * e * t[..., None]).sum(-1)
    fx, fo = inx.double() / (t * xc), inom.double() / (t * om)
    dprob, m_dprob = s_k * fx + s_k * fo, m_sk * (fx + fo)                          # s_nk = -s_k
    dtt, m_dtt = -(s_y / (t * t)) * span, m_sy / (t * t) * span
    ps, ts = (p0 + p1) ** 2, (t0 + t1) ** 2
    ref = torch.stack([dprob * p1 / ps, -dprob * p0 / ps, dtt * t1 / ts, -dtt * t0 / ts], -1)
    mag = torch.stack([m_dprob * p1 / ps, m_dprob * p0 / ps, m_dtt * t1 / ts, m_dtt * t0 / ts], -1)
    cls = torch.where(~inx, X_CLAMP, torch.where(~inom, OM_CLAMP, torch.where(t < COLD_BELOW, COLD, ORDINARY)))
    return dict(d_pt=(ref, mag), d_cup=(probs * g, g.abs() * m_probs), cls=cls, r=r, probs=probs, depth_rel=depth_rel[..., 0])


def logbinom_bwd_f32(pt, centers, gd, min_temp=MIN_TEMP, max_temp=MAX_TEMP, naive=False):
    """the kernel's arithmetic in numpy float32, operation by operation -> (d_pt [B,h,w,4], d_cup [B,h,w,nb]).  naive=True (planted defect): the
    full-size form, softmax of y / t and sums of dz_k k, dz_k (n - 1 - k), dz_k y_k"""
    with np.errstate(under="ignore"):
        q = _np32(pt)[..., :4] + E4
        p0, p1, t0, t1 = (q[..., i] for i in range(4))
        lo, hi = f32(min_temp), f32(max_temp)
        prob, tt = p0 / (p0 + p1), t0 / (t0 + t1)
        t = (hi - lo) * tt + lo
        om_raw = f32(1) - prob
        om, xc = np.minimum(np.maximum(om_raw, E4), f32(1)), np.minimum(np.maximum(prob, E4), f32(1))
        lp, lq = np.log(xc), np.log(om)
        nb = centers.shape[-1]
        logc = logc_table(nb).numpy()
        k = np.arange(nb, dtype=f32)
        B, h, w = prob.shape
        c = bilerp_f32(_np32(centers), h, w)
        g = _np32(gd)[..., None]
        y = (logc + k * lp[..., None]) + (f32(nb - 1) - k) * lq[..., None]
        z = y / t[..., None]
        assert z.dtype == f32
        if naive:
            pe = np.exp(z - z.max(-1, keepdims=True))
            pr = pe / pe.sum(-1, keepdims=True, dtype=f32)
            depth = (pr * c).sum(-1, keepdims=True, dtype=f32)
            dz = pr * (c - depth) * g
            s_k, s_nk, s_y = (dz * k).sum(-1, dtype=f32), (dz * (f32(nb - 1) - k)).sum(-1, dtype=f32), (dz * y).sum(-1, dtype=f32)
        else:
            r = (nb - 1) - np.flip(z, -1).argmax(-1)
            kr = k - r[..., None].astype(f32)
            cr, lcr = np.take_along_axis(c, r[..., None], -1), logc[r][..., None]
            yr = (logc - lcr) + kr * (lp - lq)[..., None]
            pe = np.exp(yr / t[..., None])
            cc = c - cr
            den = pe.sum(-1, keepdims=True, dtype=f32)
            depth = (pe * cc).sum(-1, keepdims=True, dtype=f32) / den
            pr = pe / den
            dz = pr * (cc - depth) * g
            s_k, s_y = (dz * kr).sum(-1, dtype=f32), (dz * yr).sum(-1, dtype=f32)
            s_nk = -s_k
        inx, inom = (prob >= E4) & (prob <= 1), (om_raw >= E4) & (om_raw <= 1)
        dprob = np.where(inx, (s_k / t) / xc, f32(0)) - np.where(inom, (s_nk / t) / om, f32(0))
        dtt = -(s_y / (t * t)) * (hi - lo)
        ps, ts = (p0 + p1) * (p0 + p1), (t0 + t1) * (t0 + t1)
        d_pt = np.stack([dprob * p1 / ps, -dprob * p0 / ps, dtt * t1 / ts, -dtt * t0 / ts], -1)
        d_cup = pr * g
    assert d_pt.dtype == f32 and d_cup.dtype == f32
    return torch.from_numpy(d_pt), torch.from_numpy(d_cup)


def logbinom_bwd_torch(pt, centers, gd, min_temp=MIN_TEMP, max_temp=MAX_TEMP):
    """torch float32 autograd through the naive form (head_bwd_ref.logbinom_fwd_up after pf_oracle.up): the comparator of the old test, which
    fails the element-wise bar itself -> (d_pt, d_centers_up)"""
    from oracle import pf_oracle
    from tests import head_bwd_ref as R
    p = pt[..., :4].detach().clone().requires_grad_(True)
    cu = pf_oracle.up(centers.permute(0, 3, 1, 2), pt.shape[1:3]).permute(0, 2, 3, 1).detach().requires_grad_(True)
    R.logbinom_fwd_up(p, cu, min_temp, max_temp).backward(gd)
    return p.grad, cu.grad


def logbinom_mp(pt4, taps, nb, g, min_temp=MIN_TEMP, max_temp=MAX_TEMP, digits=50):
    """one pixel at `digits` decimal digits (mpmath), full-size form: pt4 = the four float32 numbers, taps = [(weight l (exact float), float32
    centres [nb]) x 4] of the blend -> (d_pt [4], d_cup [nb]) as floats"""
    import mpmath as mp
    mp.mp.dps = digits
    M = mp.mpf
    p0, p1, t0, t1 = (M(float(f32(v) + E4)) for v in pt4)
    lo, hi = M(float(f32(min_temp))), M(float(f32(max_temp)))
    prob, t = p0 / (p0 + p1), (hi - lo) * (t0 / (t0 + t1)) + lo
    om_raw = 1 - prob
    e4 = M(float(E4))
    xc, om = min(max(prob, e4), M(1)), min(max(om_raw, e4), M(1))
    logc = [M(float(v)) for v in logc_table(nb)]
    (wy0, wx0, v00), (_, wx1, v01), (wy1, _, v10), (_, _, v11) = taps
    wy0, wy1, wx0, wx1 = M(wy0), M(wy1), M(wx0), M(wx1)
    c = [wy0 * (wx0 * M(float(v00[j])) + wx1 * M(float(v01[j]))) + wy1 * (wx0 * M(float(v10[j])) + wx1 * M(float(v11[j]))) for j in range(nb)]
    y = [logc[j] + j * mp.log(xc) + (nb - 1 - j) * mp.log(om) for j in range(nb)]
    zm = max(y) / t
    pe = [mp.exp(v / t - zm) for v in y]
    den = mp.fsum(pe)
    pr = [v / den for v in pe]
    depth = mp.fsum(a * b for a, b in zip(pr, c))
    gg = M(float(g))
    dz = [pr[j] * (c[j] - depth) * gg for j in range(nb)]
    s_k, s_nk, s_y = mp.fsum(dz[j] * j for j in range(nb)), mp.fsum(dz[j] * (nb - 1 - j) for j in range(nb)), mp.fsum(dz[j] * y[j] for j in range(nb))
    dprob = (s_k / t / xc if e4 <= prob <= 1 else 0) - (s_nk / t / om if e4 <= om_raw <= 1 else 0)
    dtt = -(s_y / (t * t)) * (hi - lo)
    ps, ts = (p0 + p1) ** 2, (t0 + t1) ** 2
    return [float(dprob * p1 / ps), float(-dprob * p0 / ps), float(dtt * t1 / ts), float(-dtt * t0 / ts)], [float(v * gg) for v in pr]


def pixel_taps(centers, h, w, b, oy, ox):
    """the four (ly, lx, centres) taps of pixel (b, oy, ox) for logbinom_mp, in the order 00, 01, 10, 11 (weights exact floats)"""
    (y0, y1, ly), (x0, x1, lx) = ac_taps(centers.shape[1], h), ac_taps(centers.shape[2], w)
    ly1, lx1 = float(ly[oy]), float(lx[ox])
    ly0, lx0 = 1.0 - ly1, 1.0 - lx1                                                # exact in float64 (l1 is a float32 number in [0, 1))
    cc = centers.detach().cpu()
    return [(ly0, lx0, cc[b, y0[oy], x0[ox]]), (ly0, lx1, cc[b, y0[oy], x1[ox]]), (ly1, lx0, cc[b, y1[oy], x0[ox]]), (ly1, lx1, cc[b, y1[oy], x1[ox]])]


# ---------------- activations ----------------
SQRT_HALF, INV_SQRT_2PI = math.sqrt(0.5), 1.0 / math.sqrt(2.0 * math.pi)


def act_bwd_ref(dy, v, act, pre=None):
    """dy, v [..., C] -> (ref, mag) of dy act'(.):
      relu      v = the output: dy [v > 0]; mag = |dy| [v > 0] (an element with v <= 0, -0.0 included, is exactly 0)
      softplus  v = the stored float32 output y, pre = the pre-activation x: truth dy sigmoid(x) in float64 from x.  The kernel sees only y and
                forms 1 - e^-y as -expm1(-y), one term of size |d| (softplus has no near-identity region here: d -> e^x, not 1 - 1, at small y);
                y is rounded, so d carries its sensitivity y e^-y:  mag = |dy| (|d| + y e^-y + 2^-102), d = 1 - e^-y; the last term is the
                underflow floor (an output below 2^-126 is stored as 0 or a subnormal: pre-activation -110 gives y = 0 and d = 0 exactly, against
                sigmoid(-110) = 1.7e-48)
      gelu      v = the pre-activation: dy (0.5 + 0.5 erf(v / sqrt 2) + v phi(v)); mag = |dy| (0.5 + 0.5 |erf| + |v| phi(v))"""
    d, vv = _d(dy), _d(v)
    if act == "relu":
        on = (vv > 0).double()
        return d * on, d.abs() * on
    if act == "softplus":
        dd = -torch.expm1(-vv)
        truth = torch.sigmoid(_d(pre)) if pre is not None else dd
        return d * truth, d.abs() * (dd.abs() + vv.abs() * torch.exp(-vv) + 2.0 ** -102)
    if act == "gelu":
        erf, phi = torch.erf(vv * SQRT_HALF), INV_SQRT_2PI * torch.exp(-0.5 * vv * vv)
        return d * (0.5 * (1 + erf) + vv * phi), d.abs() * (0.5 + 0.5 * erf.abs() + vv.abs() * phi)
    raise ValueError(act)


def softplus_out(x):
    """the float32 output y = fl32(log(1 + e^x)) of float32 pre-activations x, rounded once from float64 (exactly 0 below about -104)"""
    xd = _d(x)
    return torch.logaddexp(xd, torch.zeros_like(xd)).float()


def act_bwd_f32(dy, v, act, relu_ge=False):
    """Planted defect: relu_ge passes the gradient at v >= 0"""
    d, vv = _np32(dy), _np32(v)
    with np.errstate(under="ignore"):
        if act == "relu":
            dd = np.where(vv >= 0 if relu_ge else vv > 0, f32(1), f32(0))
        elif act == "softplus":
            dd = -np.expm1(-vv)
        else:
            erf = torch.erf(torch.from_numpy(vv * f32(0.70710678118654752440))).numpy()
            dd = f32(0.5) * (f32(1) + erf) + vv * f32(0.3989422804014327) * np.exp(f32(-0.5) * vv * vv)
    assert dd.dtype == f32
    return torch.from_numpy(d * dd)


def act_bwd_torch(dy, pre, act):
    """torch float32 autograd of the activation at the pre-activation, on dy's device"""
    z = pre.detach().clone().requires_grad_(True)
    {"relu": torch.relu, "softplus": F.softplus, "gelu": F.gelu}[act](z).backward(dy)
    return z.grad


# ---------------- SILog ----------------
def silog_bwd_ref(pred, target, lo=LO, hi=HI, beta=0.15, d_loss=1.0):
    """pred, target float32 of one shape -> (ref, mag): pe = fl32(pred + 1e-7f), te = fl32(target + 1e-7f), g = log pe - log te over the mask
    lo < target < hi (float32 comparisons), mean, unbiased variance, R = sqrt(var + beta mean^2), kv = 10 d_loss / R / (n - 1),
    km = 10 d_loss / R beta mean / n:   d = ((g - mean) kv + km) / pe,   mag = ((|log pe| + |log te| + |mean|) |kv| + |km|) / pe.
    At most one valid pixel, or R = 0: all zeros (mag 0)"""
    p, t = _np32(pred), _np32(target)
    m = torch.from_numpy((t > f32(lo)) & (t < f32(hi)))
    n = int(m.sum())
    pe, te = torch.from_numpy((p + E7).astype(np.float64)), torch.from_numpy((t + E7).astype(np.float64))
    zero = torch.zeros_like(pe)
    if n <= 1:
        return zero, zero.clone()
    lpe, lte = torch.log(pe), torch.log(torch.where(m, te, torch.ones_like(te)))
    g = lpe - lte
    gm = g[m]
    mean = gm.sum() / n
    var = (((gm - mean) ** 2).sum() / (n - 1)).clamp_min(0)
    b, dl = float(f32(beta)), float(f32(d_loss))
    R = torch.sqrt(var + b * mean * mean)
    if float(R) == 0.0:
        return zero, zero.clone()
    k0 = 10.0 * dl / R
    kv, km = k0 / (n - 1), k0 * b * mean / n
    ref = torch.where(m, ((g - mean) * kv + km) / pe, zero)
    mag = torch.where(m, ((lpe.abs() + lte.abs() + mean.abs()) * kv.abs() + km.abs()) / pe, zero)
    return ref, mag


def silog_bwd_f32(pred, target, lo=LO, hi=HI, beta=0.15, d_loss=1.0, mask_le=False):
    """the kernel's arithmetic: float32 g, float64 sums and scalars, one rounding of the quotient.  Planted defect: mask_le takes lo <= target <= hi"""
    p, t = _np32(pred), _np32(target)
    m = ((t >= f32(lo)) & (t <= f32(hi))) if mask_le else ((t > f32(lo)) & (t < f32(hi)))
    pe = p + E7
    with np.errstate(invalid="ignore", divide="ignore"):
        g = np.log(pe) - np.log(np.where(m, t, f32(1)) + E7)
    assert g.dtype == f32
    g64 = g.astype(np.float64)
    cnt, s1, s2 = float(m.sum()), float(g64[m].sum()), float((g64[m] ** 2).sum())
    out = np.zeros_like(p)
    if cnt > 1:
        mean = s1 / cnt
        var = max((s2 - s1 * s1 / cnt) / (cnt - 1), 0.0)
        R = math.sqrt(var + float(f32(beta)) * mean * mean)
        k0 = 10.0 * float(f32(d_loss)) / R if R > 0 else 0.0
        kv, km = k0 / (cnt - 1), k0 * float(f32(beta)) * mean / cnt
        out = np.where(m, (((g64 - mean) * kv + km) / pe.astype(np.float64)).astype(f32), f32(0))
    return torch.from_numpy(out)


def silog_bwd_torch(pred, target, lo=LO, hi=HI, beta=0.15, d_loss=1.0):
    """torch float32 autograd through pf_oracle.silog_loss on pred's device"""
    from oracle import pf_oracle
    p = pred.detach().clone().requires_grad_(True)
    loss = pf_oracle.silog_loss(p, target, lo, hi, beta)
    (loss.sum() * float(f32(d_loss))).backward()
    return p.grad


# ---------------- grading ----------------
def old_bar(y, truth, comp):
    """the tensor-normwise bar of tests/test_head_bwd_kernels_gpu.py: max |g - g64| / max |g64| <= 2 x the comparator's + 4 2^-24"""
    nw = lambda v: float("inf") if not torch.isfinite(_d(v)).all() else float((_d(v) - truth).abs().max() / max(float(truth.abs().max()), TINY))
    return nw(y) <= 2 * nw(comp) + FLOOR


def graded(y, ybase, ref, mag):
    """-> (ok, e, base, ratio): f64_image_ref.baseline_bar on the (element-wise, normwise) errors of y against those of the float32 baseline, the
    baseline floored at 4 2^-24; ratio = the larger of e / (2 max(base, floor)) over the two errors"""
    e, b = errors(y, ref, mag), errors(ybase, ref, mag)
    ratio = max(e[0] / (2 * max(b[0], FLOOR)), e[1] / (2 * max(b[1], FLOOR)))
    return baseline_bar(e, b), e, b, ratio


def zero_mag_exact(y, ref, mag):
    """every element with mag == 0 equals ref bit for value (0.0, or init under accumulate)"""
    z = mag == 0
    return bool((_d(y)[z] == ref[z]).all())


# ---------------- cases ----------------
def nan_padded(t, pad, ld=None):
    """t [..., C] as channels [0, C) of a NaN-filled buffer [..., C + pad] (or [..., ld]) -> (buffer, view)"""
    C = t.shape[-1]
    buf = torch.full((*t.shape[:-1], ld or C + pad), float("nan"), dtype=t.dtype)
    buf[..., :C] = t
    return buf, buf[..., :C]


WGRAD_SHAPES = [(5, 3), (17, 65), (65, 65), (100, 17), (64, 64)]          # (K, N)
WGRAD_P = [1, 31, 32, 33, 97]
WGRAD_ROWS = [0, 32, 33]
X_PAD, DY_PAD = 3, 5


def wgrad_case(K, N, P, spread=False):
    """-> (x [P, K], dy [P, N]) float32; spread: dy's COLUMNS scaled over six decades, so one column's wrong scale shows element by element"""
    g = torch.Generator().manual_seed(K * 1000 + N * 10 + P)
    x = torch.randn(P, K, generator=g)
    dy = torch.randn(P, N, generator=g) * (torch.rand(P, 1, generator=g) * 3)
    if spread:
        dy = (dy.double() * decade_spread(N, 1e-3, 1e3, K + N)).float()
    return x, dy


# (src, dst): upscale (taps differ from float64's), downscale (zero-gradient sources), degenerate axes, identity
RESIZE_CASES = [((24, 32), (96, 128)), ((7, 11), (96, 128)), ((33, 49), (17, 25)), ((96, 128), (24, 32)), ((5, 7), (1, 1)), ((1, 1), (4, 4)),
                ((1, 9), (6, 9)), ((5, 7), (5, 7))]
RESIZE_C, RESIZE_LD = 5, 8
RESIZE_STRIDE = ((820, 1024), (410, 512))                                  # dx [1, 820, 1024, 5]: 4 198 400 elements, 4096 past ELEM_CAPACITY


def resize_case(src, dst, B=2):
    g = torch.Generator().manual_seed(17 + src[0] + 3 * dst[1])
    return torch.randn(B, *dst, RESIZE_C, generator=g), torch.randn(B, *src, RESIZE_C, generator=g)     # dy, init


ATTR_BINS = [1, 63, 64, 65, 129, 256]
ATTR_NATTR = [1, 3, 16]
ATTR_GRIDS = {"up": ((2, 5, 7), (3, 5)), "prev_1x1": ((2, 5, 7), (1, 1)), "out_1x1": ((2, 1, 1), (3, 5)), "same": ((2, 5, 7), (5, 7))}
ATTR_STRIDE = ((1, 331, 199), (5, 7))                                      # 65 869 pixels: PIXEL_CAPACITY + 333
A_PAD = 8


def attractor_case(n_bins, n_attr, grid="up", shape=None):
    """A [B,h,w,n_attr] and b_prev [B,hp,wp,n_bins] uniform in [0, 0.5) as in tests/test_head_bwd_ref_cpu.attractor_case: close enough that
    300 dx^2 passes through 1 (f' changes sign); g ~ N(0, 1).  The elements are ill-conditioned in c (mag / |ref| up to 60), so the NORMWISE error of
    a tensor is set by the rounding of one blend times f'': with its own, equally valid float32 blend the numpy restatement lies above twice torch's in
    1 to 5 % of the gradings over seeds (element-wise it never passes half the bar).  The seed offset 22 is one at which it lies below at every case."""
    (B, h, w), (hp, wp) = shape or ATTR_GRIDS[grid]
    g = torch.Generator().manual_seed(22 + n_attr + 7 * n_bins + h)
    return (torch.rand(B, h, w, n_attr, generator=g) * 0.5, torch.rand(B, hp, wp, n_bins, generator=g) * 0.5, torch.randn(B, h, w, n_bins, generator=g))


LB_BINS = [2, 63, 64, 65, 256]
LB_KINDS = {"own": 1.0, "cold": 0.002, "hot": 20.0}                        # factor on pt[..., 2]
LB_CEN_GRIDS = {"5x7": (5, 7), "own_grid": (9, 13), "1x1": (1, 1)}
LB_SHAPE = (2, 9, 13)
LB_STRIDE = (1, 331, 199)


def logbinom_case(n_bins, kind="own", cen_grid=(5, 7), shape=LB_SHAPE, extra_rows=True):
    """tests/test_head_bwd_ref_cpu.logbinom_case (the same numbers at n_bins = 64, 'own', (5, 7), extra_rows=False: rows 0 / 1 of every image below /
    above the two clamps, temperatures around 4) with further rows: row 2 prob = 1e-3 (peak at bin 0, no clamp), row 3 prob = 1 - 1e-3 (peak at the
    last bin), row 4 p0 = p1 (x = 0.5 exactly: a two-way tie of y_k / t at the middle bins of an even n_bins, the float32 table being symmetric
    there); pt[..., 2] scaled by LB_KINDS[kind] -> (pt [B,h,w,4], centres [B,hc,wc,n_bins], d_depth [B,h,w]) float32"""
    B, h, w = shape
    g = torch.Generator().manual_seed(7)
    pt = torch.rand(B, h, w, 4, generator=g, dtype=F64) * 2 + 0.05
    pt[:, 0, :, 0], pt[:, 0, :, 1] = 1e-6, 30.0
    pt[:, 1, :, 0], pt[:, 1, :, 1] = 30.0, 1e-6
    pt[..., 2] *= 0.1
    cen = torch.rand(B, *cen_grid, n_bins, generator=g, dtype=F64).cumsum(-1)
    gd = torch.randn(B, h, w, generator=g, dtype=F64)
    if extra_rows:
        pt[:, 2, :, 0], pt[:, 2, :, 1] = 0.002, 2.0
        pt[:, 3, :, 0], pt[:, 3, :, 1] = 2.0, 0.002
        pt[:, 4, :, 1] = pt[:, 4, :, 0]
    pt[..., 2] *= LB_KINDS[kind]
    return pt.float(), cen.float(), gd.float()


def logbinom_cases():
    """name -> (n_bins, kind, centres grid, extra rows): every n_bins at every kind on the (5, 7) grid; the two other grids at 65 bins; the very
    numbers of tests/test_head_bwd_ref_cpu.logbinom_case"""
    cases = {f"nb{nb}_{kind}": (nb, kind, (5, 7), True) for nb in LB_BINS for kind in LB_KINDS}
    cases.update({f"nb65_own_cen_{name}": (65, "own", grid, True) for name, grid in LB_CEN_GRIDS.items() if name != "5x7"})
    cases["nb64_reference_case"] = (64, "own", (5, 7), False)
    return cases


def logbinom_operands(name):
    nb, kind, grid, extra = logbinom_cases()[name]
    return logbinom_case(nb, kind, grid, extra_rows=extra)


ACT_C, ACT_LD = 12, 16
RELU_EDGE = [0.0, -0.0, float(np.float32(1e-45)), -1.5, 2.0, float(np.float32(-1e-45))]       # outputs: +0, -0, the smallest subnormal, negatives
SOFTPLUS_EDGE = [-110.0, -20.0, 0.0, float(f32(19.9)), 25.0]                                  # pre-activations
GELU_EDGE = [-8.0, -6.0, float(f32(-0.7518)), 0.0, float(f32(0.7518)), 6.0, 8.0]
ACT_STRIDE_P = 349_600                                                      # x 12 = 4 195 200 elements: ELEM_CAPACITY + 896


def act_case(act, P=70):
    """-> (dy [P, 12], pre [P, 12] pre-activations, v [P, 12] what the kernel reads): a seeded spread 2 N(0, 1) with the edge values of the
    activation in the first and the last pixel.  relu: v = relu(pre) with RELU_EDGE written into the OUTPUT (pre = v there); softplus:
    v = softplus_out(pre); gelu: v = pre"""
    g = torch.Generator().manual_seed(23 + len(act))
    pre = torch.randn(P, ACT_C, generator=g) * 2
    dy = torch.randn(P, ACT_C, generator=g)
    edge = {"relu": RELU_EDGE, "softplus": SOFTPLUS_EDGE, "gelu": GELU_EDGE}[act]
    for row in (0, P - 1):
        pre[row, :len(edge)] = torch.tensor(edge)
    if act == "relu":
        v = torch.relu(pre)
        for row in (0, P - 1):
            v[row, :len(edge)] = torch.tensor(edge)
        return dy, v.clone(), v
    return dy, pre, (softplus_out(pre) if act == "softplus" else pre)


SILOG_STRIDE = (1, 1, 2049, 2048)                                           # 4 196 352 elements: ELEM_CAPACITY + 2048


def _silog_base(seed=29, shape=(2, 1, 9, 13)):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(*shape, generator=g) * 60 + 1, torch.rand(*shape, generator=g) * 100 - 5


def silog_cases():
    """name -> dict(pred, target, beta, d_loss, zeros): zeros = the output must be all zeros"""
    lo, hi = f32(LO), f32(HI)
    c = {}
    for beta in (0.0, 0.15, 0.85):
        pred, target = _silog_base()
        c[f"partial_beta{beta}"] = dict(pred=pred, target=target, beta=beta)
    pred, target = _silog_base(31)
    t = target.view(-1)
    t[0], t[1], t[2], t[3] = float(lo), float(hi), float(np.nextafter(lo, f32(1))), float(np.nextafter(hi, f32(0)))
    t[4], t[5] = float("nan"), -3.0
    c["bounds_nan_negative"] = dict(pred=pred, target=target)
    c["d_loss_-2.5"] = dict(pred=pred.clone(), target=target.clone(), d_loss=-2.5)
    pred, target = _silog_base(37)
    target = target.clamp(0.5, 70.0)
    c["pred_2x_target"] = dict(pred=2 * target, target=target, beta=0.15)
    pred, target = _silog_base(41)
    for nvalid in (0, 1, 2):
        tt = torch.full_like(target, -1.0)
        tt.view(-1)[[5, 77][:nvalid]] = torch.tensor([10.0, 33.0][:nvalid])
        c[f"valid_{nvalid}"] = dict(pred=pred.clone(), target=tt, zeros=nvalid < 2)
    c["beta0_equal_g"] = dict(pred=torch.full((2, 1, 8, 8), 4.0), target=torch.full((2, 1, 8, 8), 2.0), beta=0.0, zeros=True)
    pred, target = _silog_base(43)
    pred = (pred * decade_spread(pred.numel(), 1e-3 / 61, 1.0, 43).view(pred.shape)).float().clamp_min(1e-3)
    c["small_pred"] = dict(pred=pred, target=target)
    return {k: dict(dict(beta=0.15, d_loss=1.0, zeros=False), **v) for k, v in c.items()}


def sample_elements(total, capacity, n=4096, seed=5):
    """flat indices: the first, the last, n seeded ones, half of them at or past `capacity`"""
    g = torch.Generator().manual_seed(seed)
    a = torch.randint(0, capacity, (n // 2,), generator=g)
    b = torch.randint(capacity, total, (n // 2,), generator=g)
    return torch.unique(torch.cat([torch.tensor([0, total - 1]), a, b]))
