"""pytest -m gpu: the resize, RoI, max-pool, stitch, Swin and metric-bins kernels (csrc/imageops.hip, csrc/swin.hip) held to float64, element by
element (tests/f64_image_ref.py; the references and the bars are checked on the CPU in tests/test_f64_image_ref_cpu.py).

Every case fills its output with NaN, asserts that every element of the view it passed is finite and every channel outside it still NaN, and
prints one line `case, element-wise error, normwise error, the float32 restatement's (tests/fake_ops.py, same operands, on the GPU) errors`
(run with -s for the table).

The bar where the roundings can be counted: |y - ref| <= k 2^-24 mag at every element (f64_image_ref.counted_bar), k = the roundings on the
longest path from an operand to the result, in the kernel's evaluation order; bf16 inputs are exact operands.
  * bilinear (resize, resize_concat, resize_bilinear_f32, crop_resize): bilerp = ly.l0 (lx.l0 v00 + lx.l1 v01) + ly.l1 (lx.l0 v10 + lx.l1 v11)
    with l1 = src - i0 exact and l0 = 1 - l1 rounded.  Path of v00: lx.l0 (1), lx.l0 v00 (2), the inner sum (3), ly.l0 (4), its product (5), the
    outer sum (6): k = 6; the other three taps have five or four.  `add`: one more sum over everything, k = 7 with mag + |add|.
  * stitch_init: pred = depth mask, k = 1; count = mask, exact.  stitch_finish_init: pred / count, k = 1.
  * stitch_update: (d m + c a) / (c + m): a product (1), the sum of the numerator (2), the sum of the denominator (3), the quotient (4): k = 4 with
    mag = (|d m| + |c a|) / (c + m) (a fused multiply-add only removes one); count = c + m, k = 1.  Elements outside the patch: mag = 0, unchanged.
  * swin_unpartition_add: shortcut + proj, k = 1.
  * a bf16 output adds its rounding to nearest: half a bf16 ulp of the value, 2^(floor(log2 |v|) - 8).  (bfloat16 keeps 8 significant bits: that
    is 2^-8 |v| at the bottom of a binade and 2^-9 |v| only at its top, so `2^-9 |ref|` fails a correctly rounded result -- the CPU test holds
    torch's own float32 -> bf16 cast to this bar.)
  * nearest resize and maxpool2 select: bit-equal.
Elsewhere (roi_align: sample weights formed and summed in float32; LayerNorm-partition, window attention, attractor, log-binomial: sums of many terms
and exp / log) the float32 restatement on the same operands is the baseline: element-wise and normwise error each at most twice the baseline's, the
baseline floored at 4 * 2^-24 (f64_image_ref.baseline_bar); no cap taken from a measured kernel error."""
import functools

import pytest
import torch

from tests import f64_image_ref as I
from tests import test_f64_image_ref_cpu as C
from tests.fake_ops import ops as fake

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
F32, BF16 = torch.float32, torch.bfloat16
DTYPES = pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
LOG = []


def _hip():
    from patchfusion_amd.hip_ops import ops
    return ops


def _log(line):
    """one line of the per-case error table (printed: run with -s)"""
    print(line)
    LOG.append(line)


def _nan(shape, dt=F32):
    return torch.full(shape, NAN, dtype=dt, device=DEV)


def _written(buf, lo=0, hi=None):
    hi = buf.shape[-1] if hi is None else hi
    assert torch.isfinite(buf[..., lo:hi]).all(), "an element inside the view is not finite"
    assert torch.isnan(buf[..., :lo]).all() and torch.isnan(buf[..., hi:]).all(), "channels outside the view were written"


def _line(case, y, ref, mag, ybase):
    e, b = I.errors(y, ref, mag), I.errors(ybase, ref, mag)
    return e, b, f"{case:46s} elem {e[0]:.2e} norm {e[1]:.2e} | baseline elem {b[0]:.2e} norm {b[1]:.2e}"


def _counted(case, y, ref, mag, k, bf, ybase):
    ok, worst = I.counted_bar(y, ref, mag, k, bf)
    e, b, line = _line(case, y, ref, mag, ybase)
    _log(f"{line} | counted k={k}: worst |d| / bound {worst:.2f}")
    assert ok, (case, worst, e, b)


def _graded(case, y, ref, mag, ybase):
    e, b, line = _line(case, y, ref, mag, ybase)
    _log(line)
    assert I.baseline_bar(e, b), (case, e, b)
    return e, b


def _tag(dt):
    return "bf16" if dt == BF16 else "f32"


# ---------------- bilinear resize ----------------
@functools.lru_cache(maxsize=None)
def _resize_operands(case, dt):
    """operands, float64 references and the restatement's outputs of a case: computed once, shared by both kernel versions"""
    h, w, oh, ow, Cc = case
    x, add = I.features((2, h, w, Cc), h, dt), I.features((2, oh, ow, Cc), w + 1, dt)
    refs = (I.bilinear_ref(x, oh, ow), I.bilinear_ref(x, oh, ow, add), I.resize_concat_ref([x, add, x], oh, ow))
    x, add = x.to(DEV), add.to(DEV)
    b0, b1, b2 = _nan((2, oh, ow, Cc), dt), _nan((2, oh, ow, Cc), dt), _nan((2, oh, ow, 3 * Cc), dt)
    fake.resize(x, b0)
    fake.resize(x, b1, add=add)
    fake.resize_concat([x, add, x], b2)
    return x, add, refs, (b0.cpu(), b1.cpu(), b2.cpu())


@pytest.mark.parametrize("v2", ["1", "0"], ids=["v2", "v1"])
@DTYPES
@pytest.mark.parametrize("case", I.RESIZE_CASES, ids=lambda c: "x".join(map(str, c)))
def test_bilinear_resize_counted(monkeypatch, case, dt, v2):
    """PF_RESIZE_V2=1: the source-aligned kernel (the last case is above its LDS-table limit and falls through); 0: the output-walking kernels"""
    monkeypatch.setenv("PF_RESIZE_V2", v2)
    h, w, oh, ow, Cc = case
    x, add, refs, base = _resize_operands(case, dt)
    bf = dt == BF16
    name = f"resize_{'x'.join(map(str, case))}_{_tag(dt)}_v{2 if v2 == '1' else 1}"
    buf = _nan((2, oh, ow, Cc + 16), dt)
    _hip().resize(x, buf[..., 8:8 + Cc])
    torch.cuda.synchronize()
    _written(buf, 8, 8 + Cc)
    _counted(name, buf[..., 8:8 + Cc], *refs[0], I.K_BILERP, bf, base[0])
    y = _nan((2, oh, ow, Cc), dt)
    _hip().resize(x, y, add=add)
    torch.cuda.synchronize()
    _written(y)
    _counted(name + "_add", y, *refs[1], I.K_BILERP_ADD, bf, base[1])
    buf = _nan((2, oh, ow, 3 * Cc + 16), dt)
    _hip().resize_concat([x, add, x], buf[..., 8:8 + 3 * Cc])
    torch.cuda.synchronize()
    _written(buf, 8, 8 + 3 * Cc)
    _counted(name + "_concat3", buf[..., 8:8 + 3 * Cc], *refs[2], I.K_BILERP, bf, base[2])


@pytest.mark.parametrize("h,w,oh,ow", I.PLANE_CASES)
def test_planar_resizes(h, w, oh, ow):
    x = I.features((h, w, 1), h)[..., 0].contiguous()
    xd = x.to(DEV)
    ref, mag = I.bilinear_plane_ref(x, oh, ow)
    y, yb = _nan((oh, ow)), _nan((oh, ow))
    _hip().resize_bilinear_f32(xd, y)
    fake.resize_bilinear_f32(xd, yb)
    torch.cuda.synchronize()
    _written(y)
    _counted(f"resize_bilinear_f32_{h}x{w}_{oh}x{ow}", y, ref, mag, I.K_BILERP, False, yb)
    y = _nan((oh, ow))
    _hip().resize_nearest_f32(xd, y)
    torch.cuda.synchronize()
    _written(y)
    same = torch.equal(y.cpu(), I.nearest_ref(x, oh, ow))
    _log(f"{f'resize_nearest_f32_{h}x{w}_{oh}x{ow}':46s} bit-equal {same}")
    assert same


def test_crop_resize():
    img = I.features((96, 130, 3), 5).permute(2, 0, 1).contiguous()
    boxes = torch.tensor(I.CROP_BOXES, dtype=torch.int32)
    P = len(I.CROP_BOXES)
    ref, mag = I.crop_resize_ref(img, boxes, 28, 42)
    y, yb = _nan((P, 3, 28, 42)), _nan((P, 3, 28, 42))
    _hip().crop_resize(img.to(DEV), boxes.to(DEV), y)
    fake.crop_resize(img.to(DEV), boxes.to(DEV), yb)
    torch.cuda.synchronize()
    _written(y)
    _counted("crop_resize_3x96x130_28x42", y, ref, mag, I.K_BILERP, False, yb)
    assert torch.equal(y[5].cpu(), img[:, 30:58, 50:92]), "the box of the output's size is not a copy"


# ---------------- roi_align ----------------
@DTYPES
@pytest.mark.parametrize("h,w,Cc", I.ROI_FEATS)
def test_roi_align(h, w, Cc, dt):
    """inside, touching the far corner, partly outside, wholly outside; into the upper channel half of a 2C buffer"""
    f, rois = C.roi_operands(h, w, Cc, dt, feat=False)
    ref, mag = I.roi_align_ref(f, rois, h, w, h / 112)
    f, rois = f.to(DEV), rois.to(DEV)
    buf, bb = _nan((5, h, w, 2 * Cc), dt), _nan((5, h, w, 2 * Cc), dt)
    _hip().roi_align(f, rois, buf[..., Cc:], h / 112)
    fake.roi_align(f, rois, bb[..., Cc:], h / 112)
    torch.cuda.synchronize()
    _written(buf, Cc, 2 * Cc)
    assert bool((buf[4, ..., Cc:] == 0).all()), "the RoI wholly outside the map is not zero"
    _graded(f"roi_align_{h}x{w}x{Cc}_{_tag(dt)}", buf[..., Cc:], ref, mag, bb[..., Cc:])


@DTYPES
def test_roi_align_multi_sample(dt):
    f = I.features((2, 16, 16, 8), 3, dt)
    f = (f + torch.randn(2, 16, 16, 8, generator=torch.Generator().manual_seed(3)).to(dt)).to(dt)
    r2 = torch.tensor([[1, 0.0, 0.0, 16.0, 16.0], [0, 2.0, 3.0, 14.0, 12.0]])
    ref, mag = I.roi_align_ref(f, r2, 4, 5, 1.0)
    y, yb = _nan((2, 4, 5, 8), dt), _nan((2, 4, 5, 8), dt)
    _hip().roi_align(f.to(DEV), r2.to(DEV), y, 1.0)
    fake.roi_align(f.to(DEV), r2.to(DEV), yb, 1.0)
    torch.cuda.synchronize()
    _written(y)
    _graded(f"roi_align_multi_sample_16x16x8_{_tag(dt)}", y, ref, mag, yb)


def test_roi_align_depth():
    d = torch.rand(1, 1, 112, 154, generator=torch.Generator().manual_seed(9))
    rois = torch.tensor(I.ROIS)
    ref, mag = I.roi_align_depth_ref(d, rois, 112, 154, 1.0)
    y, yb = _nan((5, 1, 112, 154)), _nan((5, 1, 112, 154))
    _hip().roi_align_depth(d.to(DEV), rois.to(DEV), y, 1.0)
    fake.roi_align_depth(d.to(DEV), rois.to(DEV), yb, 1.0)
    torch.cuda.synchronize()
    _written(y)
    _graded("roi_align_depth_112x154", y, ref, mag, yb)


# ---------------- maxpool2 ----------------
@DTYPES
def test_maxpool2_is_exact(dt):
    x = torch.randn(2, 49, 65, 32, generator=torch.Generator().manual_seed(1)).to(dt)
    buf = _nan((2, 24, 32, 48), dt)
    _hip().maxpool2(x.to(DEV), buf[..., 8:40])
    torch.cuda.synchronize()
    _written(buf, 8, 40)
    same = torch.equal(buf[..., 8:40].cpu(), I.maxpool2_ref(x))
    _log(f"{f'maxpool2_49x65x32_{_tag(dt)}':46s} bit-equal {same}")
    assert same


# ---------------- stitch ----------------
def test_stitch():
    depth, mask, rawmask, small, yx = (t.to(DEV) for t in C.stitch_operands())
    hip = _hip()
    pred, cnt, avg = _nan((56, 84)), _nan((56, 84)), _nan((56, 84))
    pb, cb, ab = _nan((56, 84)), _nan((56, 84)), _nan((56, 84))
    (rp, mp), rc = I.stitch_init_ref(pred, cnt, depth[:4], mask, yx)
    hip.stitch_init(pred, cnt, depth[:4].contiguous(), mask, yx)
    fake.stitch_init(pb, cb, depth[:4], mask, yx)
    torch.cuda.synchronize()
    _written(pred)
    _written(cnt)
    _counted("stitch_init_4x28x42_pred", pred, rp, mp, I.K_STITCH_INIT, False, pb)
    assert torch.equal(cnt.cpu().double(), rc), "count is not the mask"
    ra, ma = I.stitch_finish_ref(pred, cnt)
    hip.stitch_finish_init(avg, pred, cnt)
    fake.stitch_finish_init(ab, pred, cnt)
    torch.cuda.synchronize()
    _written(avg)
    _counted("stitch_finish_init_56x84", avg, ra, ma, I.K_DIV, False, ab)
    steps = (("interior_14_21", depth[4], mask, 14, 21), ("last_row_col_28_42", depth[5], mask, 28, 42), ("nearest_20x30_9_13", small, rawmask, 9, 13))
    for name, d, m, y0, x0 in steps:
        (ra, ma), (rc, mc) = I.stitch_update_ref(avg, cnt, d, m, y0, x0)
        ab, cb = avg.clone(), cnt.clone()
        fake.stitch_update(ab, cb, d, m, y0, x0)
        hip.stitch_update(avg, cnt, d.contiguous(), m, y0, x0)
        torch.cuda.synchronize()
        _written(avg)
        _written(cnt)
        _counted(f"stitch_update_{name}_avg", avg, ra, ma, I.K_STITCH_AVG, False, ab)
        _counted(f"stitch_update_{name}_count", cnt, rc, mc, I.K_ADD, False, cb)


# ---------------- Swin (G2L) ----------------
def _attention(case, qkv, bt, shift, dt, name):
    """-> y (device), (e, base): the window attention of a case graded against float64 and the restatement"""
    B, H, W, Cc, heads = case
    Hp, Wp = I._pad12(H), I._pad12(W)
    ref, mag = I.swin_window_attention_ref(qkv, bt, B, Hp, Wp, Cc, heads, shift)
    qd, bd = qkv.to(DEV), bt.to(DEV)
    y, yb = _nan(tuple(ref.shape), dt), _nan(tuple(ref.shape), dt)
    _hip().swin_window_attention(qd, y, bd, B, Hp, Wp, Cc, heads, shift)
    fake.swin_window_attention(qd, yb, bd, B, Hp, Wp, Cc, heads, shift)
    torch.cuda.synchronize()
    _written(y)
    return y, _graded(name, y, ref, mag, yb)


@pytest.mark.parametrize("shift", [0, 6])
@DTYPES
@pytest.mark.parametrize("case", I.SWIN_CASES, ids=lambda c: "x".join(map(str, c)))
def test_swin_kernels(case, dt, shift):
    """one case per head_dim instantiation (2, 4, 8, 16, 32); 13 x 24, 17 x 12 and 14 x 19 are padded to multiples of 12"""
    B, H, W, Cc, heads = case
    x, gam, bet, qkv, bt, proj, Hp, Wp, nt = C.swin_operands(*case, dt)
    name = f"{'x'.join(map(str, case))}_s{shift}_{_tag(dt)}"
    ref, mag = I.swin_ln_partition_ref(x, gam, bet, 1e-5, shift)
    xd, gd, bd = x.to(DEV), gam.to(DEV), bet.to(DEV)
    y, yb = _nan((nt, Cc), dt), _nan((nt, Cc), dt)
    _hip().swin_ln_partition(xd, y, gd, bd, 1e-5, shift)
    fake.swin_ln_partition(xd, yb, gd, bd, 1e-5, shift)
    torch.cuda.synchronize()
    _written(y)
    assert bool((y.cpu()[mag == 0] == 0).all()), "a padded token is not exactly zero"
    _graded("swin_ln_partition_" + name, y, ref, mag, yb)
    _attention(case, qkv, bt, shift, dt, "swin_window_attention_" + name)
    ref, mag = I.swin_unpartition_add_ref(proj, x, shift)
    buf, bb = _nan((B, H, W, Cc + 16), dt), _nan((B, H, W, Cc), dt)
    _hip().swin_unpartition_add(proj.to(DEV), xd, buf[..., 8:8 + Cc], shift)
    fake.swin_unpartition_add(proj.to(DEV), xd, bb, shift)
    torch.cuda.synchronize()
    _written(buf, 8, 8 + Cc)
    _counted("swin_unpartition_add_" + name, buf[..., 8:8 + Cc], ref, mag, I.K_ADD, dt == BF16, bb)


@DTYPES
@pytest.mark.parametrize("kind", ["plain", "logits_x4", "key_x8"])
def test_window_attention_applies_bias_and_mask(kind, dt):
    """a bias table of unit standard deviation on a padded, shifted map; qkv x 4 (logits x 16); one key of the last window x 8.  The output is more
    than 100 baseline errors away from the float64 attention without the bias, and from the one without the shift mask: both are really applied"""
    case = (1, 13, 24, 64, 8)
    B, H, W, Cc, heads = case
    x, gam, bet, qkv, bt, proj, Hp, Wp, nt = C.swin_operands(*case, F32, seed=1)
    assert 0.9 < float(bt.std()) < 1.1
    if kind == "logits_x4":
        qkv = qkv * 4
    if kind == "key_x8":
        qkv[nt - 144 + 77, Cc:2 * Cc] *= 8
    qkv = qkv.to(dt)
    y, (e, base) = _attention(case, qkv, bt, 6, dt, f"swin_window_attention_{kind}_{_tag(dt)}")
    for what, kw in (("bias", dict(use_bias=False)), ("mask", dict(use_mask=False))):
        far = I.errors(y, *I.swin_window_attention_ref(qkv, bt, B, Hp, Wp, Cc, heads, 6, **kw))
        _log(f"{f'  without the {what} in the reference':46s} elem {far[0]:.2e} norm {far[1]:.2e}")
        assert far[0] > 100 * max(base[0], I.FLOOR) and far[1] > 100 * max(base[1], I.FLOOR), (what, far, base)


# ---------------- metric-bins head ----------------
def _attractor(name, A, n_attr, bp, h, w, **kw):
    ref, mag = I.attractor_ref(A, n_attr, bp, h, w, **kw)
    Ad, bd = A.to(DEV), bp.to(DEV)
    y, yb = _nan((2, h, w, 64)), _nan((2, h, w, 64))
    _hip().attractor(Ad, n_attr, bd, y, **kw)
    fake.attractor(Ad, n_attr, bd, yb, **kw)
    torch.cuda.synchronize()
    _written(y)
    _graded(name, y, ref, mag, yb)


@pytest.mark.parametrize("n_attr,shape", C.BINS, ids=[f"n{b[0]}" for b in C.BINS])
def test_attractor(n_attr, shape):
    hp, wp, h, w = shape
    A, bp = C.attractor_operands(n_attr, hp, wp, h, w)
    _attractor(f"attractor_n{n_attr}_{hp}x{wp}_{h}x{w}", A, n_attr, bp, h, w)


@pytest.mark.parametrize("kw", C.VARIANTS, ids=["stride2_eps", "stride2_eps_exp_sum", "exp", "sum"])
def test_attractor_variants(kw):
    A, bp = C.attractor_operands(16, 8, 11, 16, 22, stride=kw.get("a_stride", 1))
    _attractor("attractor_n16_8x11_16x22_" + "_".join(f"{k}={v}" for k, v in kw.items()), A, 16, bp, 16, 22, **kw)


@pytest.mark.parametrize("ends", [False, True], ids=["random", "temperature_ends"])
def test_logbinom_depth(ends):
    """pt 2 x 56 x 77 x 4, centres 2 x 32 x 44 x 64; `temperature_ends`: t0 / (t0 + t1) is 0 in the left half and 1 in the right half of the map"""
    pt, cen = C.logbinom_operands(ends)
    ref, mag = I.logbinom_depth_ref(pt, cen, 56, 77, 0.0212, 50.0)
    y, yb = _nan((2, 56, 77)), _nan((2, 56, 77))
    _hip().logbinom_depth(pt.to(DEV), cen.to(DEV), y, 0.0212, 50.0)
    fake.logbinom_depth(pt.to(DEV), cen.to(DEV), yb, 0.0212, 50.0)
    torch.cuda.synchronize()
    _written(y)
    _graded(f"logbinom_depth_{'temperature_ends' if ends else 'random'}", y, ref, mag, yb)
