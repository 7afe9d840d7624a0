"""tests/f64_head_bwd_ref.py proved on the CPU (no GPU needed):

  * every reference equals float64 autograd through oracle/pf_oracle.py to 1e-10, at grids whose float32 source coordinates are exact (scale 0.5, 1,
    2, 4: there the float32-defined coordinate is the float64 one) and with the float32-defined constants handed to the oracle as the float64
    numbers they are; the log-binomial wherever that autograd is itself accurate (the ordinary class of the 'own' and 'hot' cases);
  * the peak-relative log-binomial reference equals an mpmath evaluation at 50 digits at a handful of pixels, one of them a one-hot pixel at which
    tests/head_bwd_ref.logbinom_bwd (full-size form, float64) has the wrong sign;
  * the float32 restatement of every kernel passes its bar at every case of the lists: the evidence that the bars can be met before any GPU run
    (baseline here: torch float32 on the CPU);
  * ten planted defects each fail the new bar; whether the old tensor-normwise bar of tests/test_head_bwd_kernels_gpu.py sees them is recorded in
    OLD_BAR_SEES (printed with -s) -- a record, not a requirement.  The log-binomial in the naive form and the resize adjoint from float64 coordinates
    pass the old bar (its truth and its comparator share the defect's form); the other eight are seen by the old bar as well, but only at these new
    cases: the old file has none with 65 or 256 bins, a 33-pixel split, a NaN pad, an output at 0 or a target on a bound."""
import numpy as np
import pytest
import torch

from oracle import pf_oracle
from tests import f64_head_bwd_ref as H
from tests import head_bwd_ref as R

F64 = torch.float64
TOL = 1e-10
OLD_BAR_SEES = {}


def rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def _record(name, new_ok, old_ok):
    OLD_BAR_SEES[name] = not old_ok
    print(f"planted defect {name}: new bar {'PASSES (!)' if new_ok else 'rejects'}, old tensor-normwise bar {'passes it' if old_ok else 'rejects'}")
    assert not new_ok, name


# ---------------- references against float64 autograd ----------------
def test_wgrad_reference_is_conv2d_autograd():
    x, dy = H.wgrad_case(17, 65, 33)
    w = torch.zeros(65, 17, 1, 1, dtype=F64, requires_grad=True)
    b = torch.zeros(65, dtype=F64, requires_grad=True)
    torch.nn.functional.conv2d(x.double().t()[None, :, :, None], w, b).backward(dy.double().t()[None, :, :, None])
    (dw, mw), (db, mb) = H.wgrad_ref(dy, x)
    assert rel(dw, w.grad.flatten(1)) <= TOL and rel(db, b.grad) <= TOL and bool((mw >= dw.abs()).all()) and bool((mb >= db.abs()).all())


@pytest.mark.parametrize("src,dst", [((3, 5), (5, 9)), ((1, 1), (4, 4)), ((5, 7), (5, 7)), ((9, 5), (3, 3)), ((1, 9), (6, 9))])
def test_resize_reference_is_autograd_where_the_float32_coordinates_are_exact(src, dst):
    dy, init = H.resize_case(src, dst)
    x = torch.zeros(2, H.RESIZE_C, *src, dtype=F64, requires_grad=True)
    pf_oracle.up(x, dst).backward(dy.double().permute(0, 3, 1, 2))
    ref, mag = H.resize_bwd_ref(dy, *src)
    assert rel(ref, x.grad.permute(0, 2, 3, 1)) <= TOL and bool((mag >= ref.abs() - 1e-12).all())
    ref2, mag2 = H.resize_bwd_ref(dy, *src, init=init)
    assert torch.equal(ref2, ref + init.double()) and torch.equal(mag2, mag + init.double().abs())


def test_resize_reference_differs_from_float64_coordinates_where_the_issue_says():
    """96x128 -> 24x32 (the adjoint of a 4x upscale): the float32 taps differ from float64's"""
    a, b = H.tap_matrix(24, 96), H.tap_matrix(24, 96, f64_coords=True)
    c, d = H.tap_matrix(32, 128), H.tap_matrix(32, 128, f64_coords=True)
    assert int((a != b).sum() + (c != d).sum()) > 0 and abs(a - b).max() < 1e-5


@pytest.mark.parametrize("at", ["inv", "exp"])
@pytest.mark.parametrize("kind", ["mean", "sum"])
def test_attractor_reference_is_autograd(at, kind):
    A, bp, g = H.attractor_case(65, 3, shape=((2, 5, 9), (3, 5)))                    # scales 0.5 and 0.5: exact coordinates
    a = A.double().permute(0, 3, 1, 2).requires_grad_(True)
    c = pf_oracle.up(bp.double().permute(0, 3, 1, 2), (5, 9)).requires_grad_(True)
    (c + pf_oracle._attractor_delta(a, c, dict(attractor_type=at, attractor_kind=kind))).backward(g.double().permute(0, 3, 1, 2))
    (dA, mA), (dB, mB) = H.attractor_bwd_ref(A, bp, g, at, kind)
    assert rel(dA, a.grad.permute(0, 2, 3, 1)) <= TOL and rel(dB, c.grad.permute(0, 2, 3, 1)) <= TOL
    assert bool((mA >= dA.abs()).all()) and bool((mB >= dB.abs() - 1e-12).all())
    # f'' is the derivative of f': a central difference
    dx = torch.linspace(-0.4, 0.4, 801, dtype=F64)
    fd = (H._fp_fpp(dx + 1e-6, at)[0] - H._fp_fpp(dx - 1e-6, at)[0]) / 2e-6
    assert float((fd - H._fp_fpp(dx, at)[1]).abs().max()) <= 1e-5


def _oracle_pt(pt):
    """float64 pt' with pt' + 1e-4 (float64) = fl32(pt + 1e-4f): the float32-defined sum handed to the float64 oracle"""
    return torch.from_numpy((H._np32(pt) + H.E4).astype(np.float64)) - 1e-4


@pytest.mark.parametrize("name", ["nb64_reference_case", "nb64_own", "nb65_own_cen_own_grid", "nb2_hot", "nb63_hot", "nb256_hot", "nb65_own_cen_1x1"])
def test_logbinom_reference_is_autograd_where_autograd_is_accurate(name):
    pt, cen, gd = H.logbinom_operands(name)
    lo, hi = float(np.float32(H.MIN_TEMP)), float(np.float32(H.MAX_TEMP))
    p = _oracle_pt(pt).requires_grad_(True)
    cu = pf_oracle.up(cen.double().permute(0, 3, 1, 2), pt.shape[1:3]).permute(0, 2, 3, 1).detach().requires_grad_(True)
    R.logbinom_fwd_up(p, cu, lo, hi).backward(gd.double())
    out = H.logbinom_bwd_ref(pt, cen, gd)
    m = out["cls"] == H.ORDINARY
    assert int(m.sum()) > 50
    # (centres at (5, 7) / (9, 13) / (1, 1) on a (9, 13) grid: scales 0.5, 1, 0 -- exact coordinates)
    assert rel(out["d_pt"][0][m], p.grad[m]) <= TOL and rel(out["d_cup"][0][m], cu.grad[m]) <= TOL
    assert torch.equal(H.logc_table(64), (lambda k, n: n * torch.log(n) - k * torch.log(k) - (n - k) * torch.log(n - k + 1e-7))(
        torch.arange(64, dtype=torch.float32) + 1e-7, torch.full((1,), 63.0) + 1e-7))


def test_logbinom_cases_hold_what_their_names_say():
    for name, (nb, kind, grid, extra) in H.logbinom_cases().items():
        pt, cen, gd = H.logbinom_operands(name)
        out = H.logbinom_bwd_ref(pt, cen, gd)
        cls, r = out["cls"], out["r"]
        assert bool((cls[:, 0] == H.X_CLAMP).all()) and bool((cls[:, 1] == H.OM_CLAMP).all())
        assert bool((r[:, 0] == 0).all()) and bool((r[:, 1] == nb - 1).all())
        if extra:
            assert bool((r[:, 2] == 0).all()) and bool((r[:, 3] == nb - 1).all()) and bool((cls[:, 2:4] != H.X_CLAMP).all())
            if nb % 2 == 0 and nb > 2:                                              # the two-way tie: the float32 y_k / t are EQUAL at the middle bins
                y = (H.logc_table(nb).numpy() + np.arange(nb, dtype=np.float32) * np.log(np.float32(0.5))) \
                    + (np.float32(nb - 1) - np.arange(nb, dtype=np.float32)) * np.log(np.float32(0.5))
                assert y.dtype == np.float32 and y[nb // 2 - 1] == y[nb // 2] == y.max()
                assert bool((r[:, 4] == nb // 2).all())                             # ties go to the highest bin
        if kind == "cold":
            assert bool((cls[:, 2:] == H.COLD).all()) and float(out["probs"].amax(-1)[:, :2].min()) > 0.999     # rows 0 / 1: one-hot
        if kind == "hot":
            assert not bool((cls == H.COLD).any())


def _mp_pixel(pt, cen, gd, b, oy, ox):
    nb = cen.shape[-1]
    return H.logbinom_mp(pt[b, oy, ox].tolist(), H.pixel_taps(cen, pt.shape[1], pt.shape[2], b, oy, ox), nb, float(gd[b, oy, ox]))


def test_logbinom_reference_against_mpmath_and_the_full_size_form_has_the_wrong_sign_at_a_one_hot_pixel():
    pt, cen, gd = H.logbinom_operands("nb64_cold")
    out = H.logbinom_bwd_ref(pt, cen, gd)
    (ref, mag), (cref, cmag) = out["d_pt"], out["d_cup"]
    old, _ = R.logbinom_bwd(torch.from_numpy((H._np32(pt) + H.E4).astype(np.float64)) - 1e-4, cen.double(), gd.double(),
                            float(np.float32(H.MIN_TEMP)), float(np.float32(H.MAX_TEMP)))
    # the one-hot pixel of row 1 (1 - x clamped, peak at bin 63, temperature 0.08, prob 0.9999966, the other bins below 2e-23): the full-size float64
    # form gives -6.3e-28 for d_pt[0] against +1.0e-29
    hot = (1, 1, 5)
    assert float(out["probs"][hot].max()) > 0.999999 and int(out["r"][hot]) == 63 and float(out["probs"][hot][:63].max()) < 1e-20
    for (b, oy, ox) in [hot, (1, 1, 10), (1, 2, 5), (0, 4, 7), (1, 6, 2), (0, 8, 12)]:
        d_pt, d_cup = (torch.tensor(v, dtype=F64) for v in _mp_pixel(pt, cen, gd, b, oy, ox))
        e = float(((ref[b, oy, ox] - d_pt).abs() / d_pt.abs().clamp_min(1e-300)).max())
        ec = float(((cref[b, oy, ox] - d_cup).abs() / d_cup.abs().clamp_min(1e-300)).max())
        print(f"pixel {(b, oy, ox)}: |ref - mp| / |mp| d_pt {e:.2e} d_cup {ec:.2e}; d_pt[0] mp {float(d_pt[0]):.3e} ref {float(ref[b, oy, ox, 0]):.3e} "
              f"head_bwd_ref {float(old[b, oy, ox, 0]):.3e}")
        assert e <= 1e-11 and ec <= 1e-11, (b, oy, ox)                             # relative to the ELEMENT, not to mag: 2^-24 is 6e-8
        assert bool((mag[b, oy, ox] >= d_pt.abs()).all()) and bool((cmag[b, oy, ox] >= d_cup.abs()).all())
    mp0 = _mp_pixel(pt, cen, gd, *hot)[0][0]
    assert mp0 > 0 and float(ref[hot][0]) > 0 and float(old[hot][0]) < 0 and abs(float(old[hot][0])) > 10 * mp0, "head_bwd_ref.logbinom_bwd: wrong sign here"
    # an ordinary pixel of the 'own' case, for the other classes
    pt, cen, gd = H.logbinom_operands("nb65_own")
    out = H.logbinom_bwd_ref(pt, cen, gd)
    for (b, oy, ox) in [(0, 5, 5), (1, 4, 0), (0, 1, 1)]:
        d_pt, d_cup = _mp_pixel(pt, cen, gd, b, oy, ox)
        assert float(((out["d_pt"][0][b, oy, ox] - torch.tensor(d_pt, dtype=F64)).abs() / out["d_pt"][1][b, oy, ox]).max()) <= 1e-12
        assert float(((out["d_cup"][0][b, oy, ox] - torch.tensor(d_cup, dtype=F64)).abs() / out["d_cup"][1][b, oy, ox]).max()) <= 1e-12


@pytest.mark.parametrize("act", ["relu", "softplus", "gelu"])
def test_act_reference_is_autograd(act):
    dy, pre, v = H.act_case(act)
    z = pre.double().requires_grad_(True)
    {"relu": torch.relu, "softplus": torch.nn.functional.softplus, "gelu": torch.nn.functional.gelu}[act](z).backward(dy.double())
    ref, mag = H.act_bwd_ref(dy, v, act, pre=pre)
    if act == "relu":                              # (the edge outputs are written into v, and pre = v: relu'(v) = [v > 0])
        assert torch.equal(ref, z.grad) and torch.equal(ref[0, :6], dy[0, :6].double() * torch.tensor([0, 0, 1, 0, 1, 0.0]))
    else:
        assert float(((ref - z.grad).abs() / (mag + 1e-300)).max()) <= TOL
    assert bool((mag >= ref.abs() * (1 - 1e-7)).all())
    if act == "softplus":
        assert float(v[0, 0]) == 0.0 and float(v[0, 4]) == 25.0 and 0 < float(v[0, 1]) < 3e-9


def _oracle_silog(c):
    pe = torch.from_numpy((H._np32(c["pred"]) + H.E7).astype(np.float64)) - 1e-7
    te = torch.from_numpy((H._np32(c["target"]) + H.E7).astype(np.float64)) - 1e-7
    te = torch.where(torch.isnan(te), te, torch.where((c["target"] > H.LO) & (c["target"] < H.HI), te, c["target"].double()))
    p = pe.requires_grad_(True)
    loss = pf_oracle.silog_loss(p, te, H.LO, H.HI, float(np.float32(c["beta"])))
    (loss.sum() * c["d_loss"]).backward()
    return p.grad


def test_silog_reference_is_autograd():
    for name, c in H.silog_cases().items():
        ref, mag = H.silog_bwd_ref(c["pred"], c["target"], beta=c["beta"], d_loss=c["d_loss"])
        if c["zeros"]:
            assert not ref.any() and not mag.any(), name
            continue
        want = _oracle_silog(c)
        assert float(((ref - want).abs() / (mag + 1e-300)).max()) <= TOL, name
        assert int((ref != 0).sum()) >= 2 and bool((mag >= ref.abs() * (1 - 1e-12)).all())
    c = H.silog_cases()["bounds_nan_negative"]
    ref, _ = H.silog_bwd_ref(c["pred"], c["target"])
    assert ref.view(-1)[:6].ne(0).tolist() == [False, False, True, True, False, False]


# ---------------- the float32 restatements pass their bars at every case ----------------
def test_wgrad_restatement_passes_at_every_case():
    worst = 0.0
    for (K, N) in H.WGRAD_SHAPES:
        for P in H.WGRAD_P:
            for spread in ((False, True) if (K, N, P) == (17, 65, 97) else (False,)):
                x, dy = H.wgrad_case(K, N, P, spread)
                (rw, mw), (rb, mb) = H.wgrad_ref(dy, x)
                bw, bb = H.wgrad_torch(dy, x)
                for rows in H.WGRAD_ROWS:
                    dw, db = H.wgrad_f32(dy, x, rows)
                    okw, *_, r1 = H.graded(dw, bw, rw, mw)
                    okb, *_, r2 = H.graded(db, bb, rb, mb)
                    worst = max(worst, r1, r2)
                    assert okw and okb, (K, N, P, rows, spread)
    print(f"wgrad restatement: worst ratio to the bar {worst:.3f}")


def test_resize_restatement_passes_at_every_case():
    for src, dst in H.RESIZE_CASES:
        dy, init = H.resize_case(src, dst)
        for acc in (None, init):
            ref, mag = H.resize_bwd_ref(dy, *src, init=acc)
            y = H.resize_bwd_f32(dy, *src, init=acc)
            ok, e, b, ratio = H.graded(y, H.resize_bwd_torch(dy, *src, init=acc), ref, mag)
            assert ok and H.zero_mag_exact(y, ref, mag), (src, dst, e, b)
            if src == dst and acc is None:
                assert torch.equal(y, dy)
    ref, mag = H.resize_bwd_ref(*[H.resize_case((33, 49), (17, 25))[0]], 33, 49)
    assert int((mag == 0).sum()) > 0, "the downscale case has sources that receive no gradient"


def test_attractor_restatement_passes_at_every_case():
    worst = 0.0
    for nb in H.ATTR_BINS:
        for na in H.ATTR_NATTR:
            for grid in (H.ATTR_GRIDS if (nb, na) == (65, 3) else ("up",)):
                A, bp, g = H.attractor_case(nb, na, grid)
                for at in ("inv", "exp"):
                    for kind in ("mean", "sum"):
                        (rA, mA), (rB, mB) = H.attractor_bwd_ref(A, bp, g, at, kind)
                        yA, yB = H.attractor_bwd_f32(A, bp, g, at, kind)
                        bA, bB = H.attractor_bwd_torch(A, bp, g, at, kind)
                        ok1, e1, b1, r1 = H.graded(yA, bA, rA, mA)
                        ok2, e2, b2, r2 = H.graded(yB, bB, rB, mB)
                        worst = max(worst, r1, r2)
                        assert ok1 and ok2, (nb, na, grid, at, kind, e1, b1, e2, b2)
    A, bp, g = H.attractor_case(64, 16)
    q = 300 * (A.double()[..., :, None] - H.bilinear_ref(bp, 5, 7)[0][..., None, :]) ** 2
    assert float(q.min()) < 0.5 and float(q.max()) > 2, "300 dx^2 passes through 1"
    print(f"attractor restatement: worst ratio to the bar {worst:.3f}")


def _lb_grade(y, out, key, k):
    """per class: (ok, worst |y - ref| / (k 2^-24 mag)) of the classes present"""
    ref, mag = out[key]
    res = {}
    for cl, nm in H.CLASS_NAMES.items():
        m = out["cls"] == cl
        if bool(m.any()):
            res[nm] = H.counted_bar(y[m], ref[m], mag[m], k)
    return res


def test_logbinom_restatement_lies_inside_the_counted_bound_at_every_case():
    worst = {}
    for name in H.logbinom_cases():
        pt, cen, gd = H.logbinom_operands(name)
        out = H.logbinom_bwd_ref(pt, cen, gd)
        d_pt, d_cup = H.logbinom_bwd_f32(pt, cen, gd)
        for key, y, k in (("d_pt", d_pt, H.K_LB_DPT), ("d_cup", d_cup, H.K_LB_DCUP)):
            for nm, (ok, w) in _lb_grade(y, out, key, k).items():
                worst[key] = max(worst.get(key, 0.0), w)
                assert ok, (name, key, nm, w)
    print("log-binomial restatement: worst |y - ref| / bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


@pytest.mark.parametrize("act", ["relu", "softplus", "gelu"])
def test_act_restatement_passes(act):
    dy, pre, v = H.act_case(act)
    ref, mag = H.act_bwd_ref(dy, v, act, pre=pre)
    y = H.act_bwd_f32(dy, v, act)
    ok, e, b, _ = H.graded(y, H.act_bwd_torch(dy, pre, act), ref, mag)
    assert ok and H.zero_mag_exact(y, ref, mag), (act, e, b)


def test_silog_restatement_passes_at_every_case():
    for name, c in H.silog_cases().items():
        kw = dict(beta=c["beta"], d_loss=c["d_loss"])
        ref, mag = H.silog_bwd_ref(c["pred"], c["target"], **kw)
        y = H.silog_bwd_f32(c["pred"], c["target"], **kw)
        assert torch.isfinite(y).all(), name
        if c["zeros"]:
            assert not y.any(), name
            continue
        ok, e, b, _ = H.graded(y, H.silog_bwd_torch(c["pred"], c["target"], **kw), ref, mag)
        assert ok and H.zero_mag_exact(y, ref, mag), (name, e, b)


# ---------------- planted defects ----------------
def test_defect_logbinom_in_the_naive_float32_form():
    pt, cen, gd = H.logbinom_operands("nb64_reference_case")
    out = H.logbinom_bwd_ref(pt, cen, gd)
    d_pt, d_cup = H.logbinom_bwd_f32(pt, cen, gd, naive=True)
    new_ok = all(ok for ok, _ in _lb_grade(d_pt, out, "d_pt", H.K_LB_DPT).values())
    t_pt, _ = R.logbinom_bwd(pt.double(), cen.double(), gd.double(), H.MIN_TEMP, H.MAX_TEMP)
    _record("logbinom_naive_form", new_ok, H.old_bar(d_pt, t_pt, H.logbinom_bwd_torch(pt, cen, gd)[0]))
    # and the comparator of the old test, torch's float32 autograd through the naive form, fails the element-wise bound itself
    assert not all(ok for ok, _ in _lb_grade(H.logbinom_bwd_torch(pt, cen, gd)[0], out, "d_pt", H.K_LB_DPT).values())


@pytest.mark.parametrize("nb,j0", [(65, 64), (256, 192)])
def test_defect_attractor_dropping_bins(nb, j0):
    A, bp, g = H.attractor_case(nb, 3)
    (rA, mA), (rB, mB) = H.attractor_bwd_ref(A, bp, g, "inv", "mean")
    yA, yB = H.attractor_bwd_f32(A, bp, g, "inv", "mean", drop_bins_from=j0)
    bA, bB = H.attractor_bwd_torch(A, bp, g, "inv", "mean")
    tA, tB = R.attractor_bwd(A.double(), bp.double(), g.double(), "inv", "mean")
    _record(f"attractor_drops_bins_from_{j0}_of_{nb}", H.graded(yA, bA, rA, mA)[0] and H.graded(yB, bB, rB, mB)[0],
            H.old_bar(yA, tA, bA) and H.old_bar(yB, tB, bB))
    assert not H.graded(yA, bA, rA, mA)[0] and not H.graded(yB, bB, rB, mB)[0]      # each output alone shows it


def test_defect_attractor_without_scale_on_mean():
    A, bp, g = H.attractor_case(64, 3)
    (rA, mA), (rB, mB) = H.attractor_bwd_ref(A, bp, g, "exp", "mean")
    yA, yB = H.attractor_bwd_f32(A, bp, g, "exp", "mean", no_scale=True)
    bA, bB = H.attractor_bwd_torch(A, bp, g, "exp", "mean")
    tA, tB = R.attractor_bwd(A.double(), bp.double(), g.double(), "exp", "mean")
    _record("attractor_mean_without_scale", H.graded(yA, bA, rA, mA)[0] and H.graded(yB, bB, rB, mB)[0], H.old_bar(yA, tA, bA) and H.old_bar(yB, tB, bB))


@pytest.mark.parametrize("defect", ["f64_coords", "short_high"])
def test_defect_resize_adjoint(defect):
    # f64_coords: the adjoint of a 4x downscale; short_high: that of a 4x upscale, where several destinations touch every source element
    src, dst = ((96, 128), (24, 32)) if defect == "f64_coords" else ((24, 32), (96, 128))
    dy, _ = H.resize_case(src, dst)
    ref, mag = H.resize_bwd_ref(dy, *src)
    y = H.resize_bwd_f32(dy, *src, **{defect: True})
    comp = H.resize_bwd_torch(dy, *src)
    _record(f"resize_adjoint_{defect}", H.graded(y, comp, ref, mag)[0], H.old_bar(y, R.resize_bwd(dy.double(), *src), comp))
    if defect == "f64_coords":                     # and on the adjoint of the 4x upscale the two sets of taps differ as well
        dy, _ = H.resize_case((24, 32), (96, 128))
        ref, mag = H.resize_bwd_ref(dy, 24, 32)
        assert not H.graded(H.resize_bwd_f32(dy, 24, 32, f64_coords=True), H.resize_bwd_torch(dy, 24, 32), ref, mag)[0]


def test_defect_wgrad_dropping_pixel_32_of_a_split():
    x, dy = H.wgrad_case(17, 65, 97)
    (rw, mw), (rb, mb) = H.wgrad_ref(dy, x)
    dw, db = H.wgrad_f32(dy, x, rows=33, drop_pixel=32)
    bw, bb = H.wgrad_torch(dy, x)
    _record("wgrad_drops_pixel_32_of_a_split", H.graded(dw, bw, rw, mw)[0] and H.graded(db, bb, rb, mb)[0],
            H.old_bar(dw, rw, bw) and H.old_bar(db, rb, bb))


def test_defect_wgrad_reading_a_pad_column_into_the_k_tail():
    x, dy = H.wgrad_case(17, 65, 33)
    xb, xv = H.nan_padded(x, H.X_PAD)
    (rw, mw), _ = H.wgrad_ref(dy, x)
    dw, _ = H.wgrad_f32(dy, x, k_tail_from=xb[:, 17])                              # the NaN pad of the new test
    finite = torch.randn(33, generator=torch.Generator().manual_seed(1))           # a finite pad, as the old test fills it
    old_dw, _ = H.wgrad_f32(dy, x, k_tail_from=finite)
    bw, _ = H.wgrad_torch(dy, x)
    _record("wgrad_reads_a_pad_column", H.graded(dw, bw, rw, mw)[0], H.old_bar(old_dw, rw, bw))
    assert not H.graded(old_dw, bw, rw, mw)[0]                                     # (a finite pad fails the element-wise bar too)


def test_defect_relu_with_greater_or_equal():
    dy, pre, v = H.act_case("relu")
    ref, mag = H.act_bwd_ref(dy, v, "relu")
    y = H.act_bwd_f32(dy, v, "relu", relu_ge=True)
    comp = H.act_bwd_torch(dy, pre, "relu")
    new_ok = H.graded(y, comp, ref, mag)[0] and H.zero_mag_exact(y, ref, mag)
    _record("relu_with_ge", new_ok, H.old_bar(y, R.act_bwd(dy.double(), v.double(), "relu"), comp))


def test_defect_silog_mask_with_less_or_equal():
    c = H.silog_cases()["bounds_nan_negative"]
    ref, mag = H.silog_bwd_ref(c["pred"], c["target"])
    y = H.silog_bwd_f32(c["pred"], c["target"], mask_le=True)
    comp = H.silog_bwd_torch(c["pred"], c["target"])
    new_ok = H.graded(y, comp, ref, mag)[0] and H.zero_mag_exact(y, ref, mag)
    _record("silog_mask_with_le", new_ok, H.old_bar(y, R.silog_bwd(c["pred"].double(), c["target"].double(), H.LO, H.HI), comp))


def test_sampling_and_capacities():
    assert H.ELEM_CAPACITY == 16384 * 256 == 4_194_304 and H.PIXEL_CAPACITY == 65_536
    (h, w), _ = H.RESIZE_STRIDE
    total = h * w * H.RESIZE_C
    idx = H.sample_elements(total, H.ELEM_CAPACITY)
    assert total > H.ELEM_CAPACITY and int(idx[0]) == 0 and int(idx[-1]) == total - 1 and int((idx >= H.ELEM_CAPACITY).sum()) >= 1500
    assert np.prod(H.ATTR_STRIDE[0]) > H.PIXEL_CAPACITY + 64 and np.prod(H.LB_STRIDE) > H.PIXEL_CAPACITY + 64
    assert H.ACT_STRIDE_P * H.ACT_C > H.ELEM_CAPACITY and np.prod(H.SILOG_STRIDE) > H.ELEM_CAPACITY
