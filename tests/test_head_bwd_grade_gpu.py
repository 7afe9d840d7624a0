"""pytest -m gpu: the head's backward kernels (csrc/head_bwd.hip) held to float64, element by element, through hip_ops.ops (tests/f64_head_bwd_ref.py:
references, magnitudes, cases and bars; proved on the CPU, planted defects included, in tests/test_f64_head_bwd_ref_cpu.py).  Style of
tests/test_eval_grade_gpu.py: every output is NaN-filled inside a guarded buffer, pad columns of strided outputs must still be NaN afterwards, pad
columns of strided inputs are NaN before the launch, every kernel is launched twice and must repeat bit for bit, every case prints one line (-s).

Bars
  * wgrad, resize adjoint, attractor, act, SILog: f64_image_ref.baseline_bar on the element-wise error max |y - ref| / mag and on the normwise error
    max |y - ref| / max |ref|, each at most twice that of torch float32 on the same device and operands (torch.matmul / autograd through
    pf_oracle's lines), the baseline floored at 4 x 2^-24.  An element with mag == 0 must equal its reference exactly.
  * log-binomial: torch's float32 autograd goes through the full-size y (hundreds) and fails the element-wise bound itself (printed per case), so
    the kernel is held to |y - ref| <= K 2^-24 mag (f64_image_ref.counted_bar), per class of pixel (ordinary, x clamp binding, 1 - x clamp
    binding, cold), K = the roundings counted on the kernel's longest path, each in units of the magnitude it acts on (logf / expf: 2, within one ulp):
      exponent (y_k - y_r) / t, units of e_k: logc_k - logc_r (1) | x and 1 - x: p_i + 1e-4f twice, their sum, the quotient (4, carried by e_k's
        sensitivity term), logf (2), lp - lq (1), (k - r) dl (1), the sum of the two parts (1) | t: t_i + 1e-4f twice, sum, quotient (4),
        max - min (1), the product (1), + min_temp (1), and the quotient by t (1): 8.  Longest: 4 + 2 + 1 + 1 + 1 + 8 = 13 (the logc path: 10).
      pe = expf (2): 13 e_k + 2.  den: sum_m probs_m (13 e_m + 2) and the sum itself, three adds over a lane's slots and six butterfly steps (9).
      pr = pe / den (1): 13 e_k + 13 sum_m probs_m e_m + 2 + 2 + 9 + 1 <= 14 (1 + e_k + sum probs e) = 14 mag_probs.
      d_centers_up = pr g (1):  K = 15.
      c_k - c_r: two blends of K_BILERP = 6 and the difference (1): 7; depth - c_r = num / den: product (1), sum (9), quotient (1) on top of probs
        (14) and the differences (7); c_k - depth (1): at most 14 on the probs part and 7 + 11 + 1 = 19 on the centres part of mag_dz;
      dz = pr (c_k - depth) g, two products (2): 21.  s_k: the product with the exact k - r (1), the sum (9): 31.
      dprob: / t (7 + 1), / xc (4 + 1): 44; the other quotient alike, the difference (1): 45; dprob p1 (1 + 1), ps = (p0 + p1)^2 (3 + 3 + 1), the
        quotient (1): K = 55.  (d_pt[2..3] through s_y: y_k - y_r carried by the e_k t term, / (t t) 15, (max - min) 2, t1 1, ts 7, two
        operations 2: not longer.)
    The numpy float32 restatement of the kernel lies at 0.13 (d_pt) and 0.34 (d_centers_up) of these bounds at the worst case (CPU test); the
    naive float32 form is 2e3 to 4e7 bounds off on d_pt.
No cap comes from the kernels' own measured error.  The worst ratio per kernel is printed by test_coverage; the record of a run on the MI355X is
profiles/head_bwd_grade.log and DESIGN.md's head-training section."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import f64_head_bwd_ref as H

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
F64 = torch.float64
GUARD = 16
LOG = []
RAN = set()                      # (kernel, case family) of everything that was graded: test_coverage
WORST = {}                       # kernel -> (ratio to its bar, case)
DONE = []

REQUIRED = ({("wgrad", s) for s in H.WGRAD_SHAPES} | {("wgrad", "decade_spread"), ("wgrad", "refusals")}
            | {("resize_bwd", c) for c in H.RESIZE_CASES} | {("resize_bwd", "grid_stride")}
            | {("attractor_bwd", nb) for nb in H.ATTR_BINS} | {("attractor_bwd", g) for g in H.ATTR_GRIDS} | {("attractor_bwd", "grid_stride")}
            | {("logbinom_bwd", n) for n in H.logbinom_cases()} | {("logbinom_bwd", "grid_stride"), ("logbinom_bwd", "refusals")}
            | {("act_bwd", a) for a in ("relu", "softplus", "gelu")} | {("act_bwd", "grid_stride")}
            | {("silog_bwd", n) for n in H.silog_cases()} | {("silog_bwd", "grid_stride")})


def _hip():
    from patchfusion_amd.hip_ops import ops
    return ops


def _log(line):
    print(line)
    LOG.append(line)


def _worst(op, ratio, case):
    if ratio > WORST.get(op, (-1.0, None))[0]:
        WORST[op] = (ratio, case)


def _guarded(shape):
    n = int(np.prod(shape))
    flat = torch.full((n + 2 * GUARD,), NAN, dtype=torch.float32, device=DEV)
    return flat, flat[GUARD:GUARD + n].view(shape)


def _guards_intact(flat):
    assert torch.isnan(flat[:GUARD]).all() and torch.isnan(flat[-GUARD:]).all(), "the kernel wrote outside its output"


def _out(shape, pad=0):
    """a NaN-filled guarded buffer [..., C + pad] and its view [..., :C]"""
    flat, buf = _guarded((*shape[:-1], shape[-1] + pad))
    return flat, buf, buf[..., :shape[-1]]


def _pads_nan(flat, buf, C):
    _guards_intact(flat)
    assert torch.isnan(buf[..., C:]).all(), "a pad column of the output was written"


def _dev_padded(t, pad):
    """t as channels [0, C) of a NaN-padded device buffer -> the view"""
    buf, _ = H.nan_padded(t, pad)
    return buf.to(DEV)[..., :t.shape[-1]]


def _twice(run):
    """launch twice into fresh NaN buffers: identical bits -> the first result"""
    a, b = run(), run()
    torch.cuda.synchronize()
    for u, v in zip(a, b):
        assert torch.equal(u.view(torch.int32), v.view(torch.int32)), "two launches differ"
    return a


def _grade(op, case, y, ybase, ref, mag):
    ok, e, b, ratio = H.graded(y, ybase, ref, mag)
    _log(f"{op:13s} {case:58s} elem {e[0]:.2e} norm {e[1]:.2e} | torch f32 elem {b[0]:.2e} norm {b[1]:.2e} | ratio to the bar {ratio:.3f}")
    _worst(op, ratio, case)
    assert ok, (op, case, e, b)
    assert H.zero_mag_exact(y, ref, mag), (op, case, "an element with no term is not exactly its reference")


# ---------------- weight gradient ----------------
def _wgrad(K, N, P, rows, spread=False):
    x, dy = H.wgrad_case(K, N, P, spread)
    xv, dv = _dev_padded(x, H.X_PAD), _dev_padded(dy, H.DY_PAD)

    def run():
        fw, dw = _guarded((N, K))
        fb, db = _guarded((N,))
        _hip().conv1x1_wgrad(dv, xv, dw, db, rows_per_block=rows)
        torch.cuda.synchronize()
        _guards_intact(fw), _guards_intact(fb)
        return dw, db

    dw, db = _twice(run)
    (rw, mw), (rb, mb) = H.wgrad_ref(dy, x)
    bw, bb = H.wgrad_torch(dv.contiguous(), xv.contiguous())
    tag = f"K={K} N={N} P={P} rows={rows}" + (" decade spread" if spread else "")
    _grade("wgrad", tag + " dW", dw, bw, rw, mw)
    _grade("wgrad", tag + " db", db, bb, rb, mb)


@pytest.mark.parametrize("K,N", H.WGRAD_SHAPES)
def test_wgrad(K, N):
    """K not a multiple of 16 (a ragged last fragment), the 1-wide tails of a second 64-tile in N and K (65), P either side of the 32-pixel step,
    rows_per_block 33: the second step of every split holds one live pixel; x / dy padded by 3 / 5 columns of NaN"""
    DONE.append(1)
    for P in H.WGRAD_P:
        for rows in H.WGRAD_ROWS:
            _wgrad(K, N, P, rows)
    RAN.add(("wgrad", (K, N)))


def test_wgrad_decade_spread():
    DONE.append(1)
    for rows in H.WGRAD_ROWS:
        _wgrad(17, 65, 97, rows, spread=True)
    RAN.add(("wgrad", "decade_spread"))


def test_wgrad_refusals():
    """N = 4097; 65 536 splits (on the workspace query alone; 65 535 are accepted); a workspace one byte short: refused, nothing written"""
    DONE.append(1)
    from patchfusion_amd import hip_ops
    from patchfusion_amd._lib import PfError
    L = hip_ops._L
    need = C.c_long(0)
    assert L.pf_conv1x1_wgrad_workspace_bytes(1, 4097, 5, 0, C.byref(need)) != 0
    with pytest.raises(PfError):
        _hip().conv1x1_wgrad(torch.zeros(1, 4097, device=DEV), torch.zeros(1, 5, device=DEV), torch.zeros(4097, 5, device=DEV))
    assert L.pf_conv1x1_wgrad_workspace_bytes(65536, 3, 5, 1, C.byref(need)) != 0
    assert L.pf_conv1x1_wgrad_workspace_bytes(65535, 3, 5, 1, C.byref(need)) == 0 and need.value == 65535 * (3 * 5 + 3) * 4
    x, dy = (t.to(DEV) for t in H.wgrad_case(5, 3, 33))
    assert L.pf_conv1x1_wgrad_workspace_bytes(33, 3, 5, 32, C.byref(need)) == 0 and need.value == 2 * (3 * 5 + 3) * 4
    ws = torch.empty(need.value // 4, device=DEV)
    fw, dw = _guarded((3, 5))
    fb, db = _guarded((3,))
    p = lambda t: C.c_void_p(t.data_ptr())
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert L.pf_conv1x1_wgrad(p(dy), 3, p(x), 5, 33, 3, 5, p(dw), p(db), p(ws), need.value - 1, 32, st) != 0
    torch.cuda.synchronize()
    assert torch.isnan(fw).all() and torch.isnan(fb).all(), "a refused call wrote"
    assert L.pf_conv1x1_wgrad(p(dy), 3, p(x), 5, 33, 3, 5, p(dw), p(db), p(ws), need.value, 32, st) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(dw).all() and torch.isfinite(db).all()
    RAN.add(("wgrad", "refusals"))


# ---------------- resize adjoint ----------------
@pytest.mark.parametrize("src,dst", H.RESIZE_CASES)
def test_resize_adjoint(src, dst):
    DONE.append(1)
    dy, init = H.resize_case(src, dst)
    dv = _dev_padded(dy, H.RESIZE_LD - H.RESIZE_C)
    for acc in (False, True):
        def run():
            flat, buf, dx = _out((2, *src, H.RESIZE_C), H.RESIZE_LD - H.RESIZE_C)
            if acc:
                dx.copy_(init)
            _hip().resize_bwd(dv, dx, accumulate=acc)
            torch.cuda.synchronize()
            _pads_nan(flat, buf, H.RESIZE_C)
            return (dx,)

        dx, = _twice(run)
        ref, mag = H.resize_bwd_ref(dy, *src, init=init if acc else None)
        base = H.resize_bwd_torch(dv.contiguous(), *src, init=init.to(DEV) if acc else None)
        _grade("resize_bwd", f"{src}->{dst} accumulate={acc}", dx, base, ref, mag)
        if src == dst and not acc:
            assert torch.equal(dx.cpu(), dy), "equal sizes: the identity, bit for bit"
    # <fwd(x), g> = <x, bwd(g)> with the project's own forward kernel, summed in float64
    g = torch.Generator().manual_seed(3)
    x8 = torch.zeros(2, *src, H.RESIZE_LD, device=DEV)                             # (the forward kernel takes multiples of 8 channels)
    x8[..., :H.RESIZE_C] = torch.randn(2, *src, H.RESIZE_C, generator=g).to(DEV)
    fwd8 = torch.full((2, *dst, H.RESIZE_LD), NAN, device=DEV)
    _hip().resize(x8, fwd8)
    x, fwd = x8[..., :H.RESIZE_C], fwd8[..., :H.RESIZE_C]
    bwd = _hip().resize_bwd(dv, torch.full((2, *src, H.RESIZE_C), NAN, device=DEV))
    lhs, rhs = float((fwd.double().cpu() * dy.double()).sum()), float((x.double().cpu() * bwd.double().cpu()).sum())
    tol = H.K_BILERP * H.U * float((x.double().cpu().abs() * H.resize_bwd_ref(dy, *src)[1]).sum())
    _log(f"resize_bwd     {src}->{dst} adjoint identity |lhs - rhs| / tolerance {abs(lhs - rhs) / tol:.3f}")
    assert abs(lhs - rhs) <= tol
    RAN.add(("resize_bwd", (src, dst)))


def test_resize_adjoint_grid_stride():
    """dx [1, 820, 1024, 5]: more elements than the 16384 x 256 one pass of the grid covers; graded in float64 at the first, the last and 4096
    seeded elements, half of them past that capacity"""
    DONE.append(1)
    (h, w), (oh, ow) = H.RESIZE_STRIDE
    total = h * w * H.RESIZE_C
    assert total > 16384 * 256 == H.ELEM_CAPACITY
    dy = torch.randn(1, oh, ow, H.RESIZE_C, generator=torch.Generator().manual_seed(19))
    dv = _dev_padded(dy, H.RESIZE_LD - H.RESIZE_C)

    def run():
        flat, dx = _guarded((1, h, w, H.RESIZE_C))
        _hip().resize_bwd(dv, dx)
        torch.cuda.synchronize()
        _guards_intact(flat)
        return (dx,)

    dx, = _twice(run)
    assert torch.isfinite(dx).all()
    idx = H.sample_elements(total, H.ELEM_CAPACITY)
    assert int((idx >= H.ELEM_CAPACITY).sum()) >= 1500
    c, sx, sy = idx % H.RESIZE_C, (idx // H.RESIZE_C) % w, idx // (H.RESIZE_C * w)
    My, Mx = torch.from_numpy(H.tap_matrix(h, oh)), torch.from_numpy(H.tap_matrix(w, ow))
    d64 = dy.double()[0]

    def sampled(v):
        t1 = (My.t() @ v.reshape(oh, ow * H.RESIZE_C)).view(h, ow, H.RESIZE_C)              # [h, ow, C]
        return (t1[sy, :, c] * Mx.t()[sx]).sum(-1)

    ref, mag = sampled(d64), sampled(d64.abs())
    base = H.resize_bwd_torch(dv.contiguous(), h, w).reshape(-1)[idx.to(DEV)]
    _grade("resize_bwd", f"grid stride {total} elements, {idx.numel()} sampled", dx.reshape(-1)[idx.to(DEV)], base, ref, mag)
    RAN.add(("resize_bwd", "grid_stride"))


# ---------------- attractor ----------------
def _attractor(case, A, bp, g, at, kind):
    n_attr = A.shape[-1]
    Av, bd, gd = _dev_padded(A, H.A_PAD), bp.to(DEV), g.to(DEV)

    def run():
        fa, ba, dA = _out(tuple(A.shape), H.A_PAD)
        fb, dB = _guarded(tuple(g.shape))
        _hip().attractor_bwd(Av, n_attr, bd, gd, dA, dB, attractor_type=at, kind=kind)
        torch.cuda.synchronize()
        _pads_nan(fa, ba, n_attr), _guards_intact(fb)
        return dA, dB

    dA, dB = _twice(run)
    (rA, mA), (rB, mB) = H.attractor_bwd_ref(A, bp, g, at, kind)
    bA, bB = H.attractor_bwd_torch(Av.contiguous(), bd, gd, at, kind)
    _grade("attractor_bwd", f"{case} {at} {kind} dA", dA, bA, rA, mA)
    _grade("attractor_bwd", f"{case} {at} {kind} d_b_c", dB, bB, rB, mB)


@pytest.mark.parametrize("n_bins", H.ATTR_BINS)
def test_attractor(n_bins):
    """the kernel holds four 64-lane slots: 1, 63, 64, 65, 129 and 256 bins; 1, 3 and 16 attractors; grid [2, 5, 7] from [2, 3, 5]"""
    DONE.append(1)
    for n_attr in H.ATTR_NATTR:
        ops = H.attractor_case(n_bins, n_attr)
        for at in ("inv", "exp"):
            for kind in ("mean", "sum"):
                _attractor(f"nb={n_bins} n_attr={n_attr}", *ops, at, kind)
    RAN.add(("attractor_bwd", n_bins))


@pytest.mark.parametrize("grid", list(H.ATTR_GRIDS))
def test_attractor_grids(grid):
    DONE.append(1)
    ops = H.attractor_case(65, 3, grid)
    for at in ("inv", "exp"):
        for kind in ("mean", "sum"):
            _attractor(f"nb=65 n_attr=3 grid {grid}", *ops, at, kind)
    RAN.add(("attractor_bwd", grid))


def test_attractor_grid_stride():
    """2 bins, 1 attractor, 65 869 pixels: more than the 16384 x 4 waves of one pass and a ragged remainder; every pixel graded"""
    DONE.append(1)
    shape = H.ATTR_STRIDE
    assert int(np.prod(shape[0])) > 16384 * 4 == H.PIXEL_CAPACITY
    _attractor("grid stride 65869 pixels nb=2 n_attr=1", *H.attractor_case(2, 1, shape=shape), "inv", "mean")
    RAN.add(("attractor_bwd", "grid_stride"))


# ---------------- log-binomial ----------------
def _logbinom(case, pt, cen, gd):
    nb = cen.shape[-1]
    pv, cd, gdev = _dev_padded(pt, 4), cen.to(DEV), gd.to(DEV)

    def run():
        fp, bp, d_pt = _out((*pt.shape[:3], 4), 4)
        fc, d_cup = _guarded((*pt.shape[:3], nb))
        _hip().logbinom_depth_bwd(pv, cd, gdev, d_pt, d_cup, H.MIN_TEMP, H.MAX_TEMP)
        torch.cuda.synchronize()
        _pads_nan(fp, bp, 4), _guards_intact(fc)
        return d_pt, d_cup

    d_pt, d_cup = _twice(run)
    out = H.logbinom_bwd_ref(pt, cen, gd)
    t_pt, t_cup = H.logbinom_bwd_torch(pv.contiguous(), cd, gdev)
    bad = []
    for key, y, comp, k in (("d_pt", d_pt, t_pt, H.K_LB_DPT), ("d_cup", d_cup, t_cup, H.K_LB_DCUP)):
        ref, mag = out[key]
        yc, cc = y.cpu(), comp.cpu()
        for cl, nm in H.CLASS_NAMES.items():
            m = out["cls"] == cl
            if not bool(m.any()):
                continue
            ok, w = H.counted_bar(yc[m], ref[m], mag[m], k)
            _, wt = H.counted_bar(cc[m], ref[m], mag[m], k)
            _log(f"logbinom_bwd  {case:30s} {key:5s} {nm:9s} |y - ref| / (K 2^-24 mag), K = {k}: {w:.3f} | torch f32 autograd {wt:.3g}")
            _worst(f"logbinom_bwd {key}", w, f"{case} {nm}")
            if not ok:
                bad.append((key, nm, w))
    assert not bad, (case, bad)


@pytest.mark.parametrize("name", list(H.logbinom_cases()))
def test_logbinom(name):
    DONE.append(1)
    from patchfusion_amd import hip_ops
    pt, cen, gd = H.logbinom_operands(name)
    assert torch.equal(hip_ops._logbinom_logc(cen.shape[-1], torch.device("cpu")), H.logc_table(cen.shape[-1])), "the reference's table is the kernel's"
    _logbinom(name, pt, cen, gd)
    RAN.add(("logbinom_bwd", name))


def test_logbinom_grid_stride():
    """2 bins, 65 869 pixels (see test_attractor_grid_stride); every pixel graded"""
    DONE.append(1)
    assert int(np.prod(H.LB_STRIDE)) > 16384 * 4 == H.PIXEL_CAPACITY
    _logbinom("grid stride 65869 pixels nb=2", *H.logbinom_case(2, "own", (5, 7), shape=H.LB_STRIDE))
    RAN.add(("logbinom_bwd", "grid_stride"))


def test_logbinom_refusals():
    DONE.append(1)
    from patchfusion_amd._lib import PfError
    z = lambda *s: torch.zeros(*s, device=DEV)
    for nb in (1, 257):
        with pytest.raises(PfError):
            _hip().logbinom_depth_bwd(z(1, 1, 2, 4) + 1, z(1, 1, 1, nb), z(1, 1, 2), z(1, 1, 2, 4), z(1, 1, 2, nb), H.MIN_TEMP, H.MAX_TEMP)
    with pytest.raises(PfError):                                                    # pt_ld = 3
        _hip().logbinom_depth_bwd(z(1, 1, 2, 3) + 1, z(1, 1, 1, 2), z(1, 1, 2), z(1, 1, 2, 4), z(1, 1, 2, 2), H.MIN_TEMP, H.MAX_TEMP)
    RAN.add(("logbinom_bwd", "refusals"))


# ---------------- activations ----------------
def _act(case, act, P):
    dy, pre, v = H.act_case(act, P)
    vv = _dev_padded(v, H.ACT_LD - H.ACT_C)
    dyd = dy.to(DEV)

    def run():
        flat, buf, out = _out((P, H.ACT_C), H.ACT_LD - H.ACT_C)
        out.copy_(dyd)
        _hip().act_bwd(out, vv, act)
        torch.cuda.synchronize()
        _pads_nan(flat, buf, H.ACT_C)
        return (out,)

    y, = _twice(run)
    ref, mag = H.act_bwd_ref(dy, v, act, pre=pre)
    _grade("act_bwd", case, y, H.act_bwd_torch(dyd, pre.to(DEV), act), ref, mag)
    return y.cpu(), dy


@pytest.mark.parametrize("act", ["relu", "softplus", "gelu"])
def test_act(act):
    """relu at outputs 0.0, -0.0, the smallest subnormal (positive: passes; negative: not) and a negative value; softplus from outputs of
    pre-activations -110 (the output, and so the derivative, is exactly 0), -20, 0, 19.9, 25, truth sigmoid(x) in float64; gelu at +-8, +-6,
    +-0.7518, 0"""
    DONE.append(1)
    y, dy = _act(f"{act} 70 x 12 in 16", act, 70)
    if act == "relu":
        for row in (0, 69):
            assert not y[row, 0] and not y[row, 1] and not y[row, 3] and not y[row, 5] and torch.equal(y[row, [2, 4]], dy[row, [2, 4]])
    if act == "softplus":
        assert not y[0, 0] and not y[69, 0] and torch.equal(y[0, 4], dy[0, 4])                # exactly 0 at -110, exactly dy at 25
    RAN.add(("act_bwd", act))


def test_act_grid_stride():
    DONE.append(1)
    assert H.ACT_STRIDE_P * H.ACT_C > 16384 * 256 == H.ELEM_CAPACITY
    _act(f"grid stride gelu {H.ACT_STRIDE_P} x 12", "gelu", H.ACT_STRIDE_P)
    RAN.add(("act_bwd", "grid_stride"))


# ---------------- SILog ----------------
def _silog(case, pred, target, beta, d_loss, zeros=False):
    pd, td = pred.to(DEV), target.to(DEV)
    loss, sums = _hip().silog_loss_saved(pd, td, H.LO, H.HI, beta)

    def run():
        flat, d = _guarded(tuple(pred.shape))
        _hip().silog_loss_bwd(pd, td, sums, d, H.LO, H.HI, beta, d_loss)
        torch.cuda.synchronize()
        _guards_intact(flat)
        return (d,)

    d, = _twice(run)
    assert torch.isfinite(d).all(), case
    if zeros:
        assert not d.any(), (case, "all zeros")
        _log(f"silog_bwd     {case:58s} all zeros, nothing non-finite")
        return
    ref, mag = H.silog_bwd_ref(pred, target, beta=beta, d_loss=d_loss)
    _grade("silog_bwd", case, d, H.silog_bwd_torch(pd, td, beta=beta, d_loss=d_loss), ref, mag)
    return d.cpu()


@pytest.mark.parametrize("name", list(H.silog_cases()))
def test_silog(name):
    DONE.append(1)
    c = H.silog_cases()[name]
    d = _silog(name, c["pred"], c["target"], c["beta"], c["d_loss"], c["zeros"])
    if name == "bounds_nan_negative":              # exactly lo, exactly hi: outside; their float neighbours: inside; NaN and negative: outside
        assert d.view(-1)[:6].ne(0).tolist() == [False, False, True, True, False, False]
    RAN.add(("silog_bwd", name))


def test_silog_grid_stride():
    DONE.append(1)
    assert int(np.prod(H.SILOG_STRIDE)) > 16384 * 256 == H.ELEM_CAPACITY
    pred, target = H._silog_base(47, H.SILOG_STRIDE)
    _silog(f"grid stride {int(np.prod(H.SILOG_STRIDE))} elements", pred, target, 0.15, 1.0)
    RAN.add(("silog_bwd", "grid_stride"))


def test_coverage():
    """every (kernel, case family) of the lists was graded -- checked when the whole module ran; prints the worst ratio per kernel"""
    for op, (ratio, case) in sorted(WORST.items()):
        _log(f"worst {op}: {ratio:.3f} of its bar at {case}")
    n_tests = (len(H.WGRAD_SHAPES) + 2 + len(H.RESIZE_CASES) + 1 + len(H.ATTR_BINS) + len(H.ATTR_GRIDS) + 1 + len(H.logbinom_cases()) + 2 + 3 + 1
               + len(H.silog_cases()) + 1)
    assert len(REQUIRED) == n_tests
    if len(DONE) >= n_tests:
        assert REQUIRED <= RAN, sorted(map(str, REQUIRED - RAN))
        assert RAN <= REQUIRED, sorted(map(str, RAN - REQUIRED))
