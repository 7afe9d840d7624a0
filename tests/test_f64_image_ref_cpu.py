"""CPU checks of the float64 image references (tests/f64_image_ref.py) and of the power of the per-element bars of
tests/test_image_grade_gpu.py to fail a kernel.

Agreement.  Each reference, rounded to float32, agrees with the float32 restatement of tests/fake_ops.py at the shapes of the GPU test.  How close:
  * bilinear resize (plain, add, concat, planar, crop), stitch, swin_unpartition_add: within the counted bar of the GPU test itself,
    k 2^-24 mag with k = 6 / 7 / 1 / 4 / 1 -- PyTorch's CPU bilinear kernel forms the same float32 source coordinate and blends with the same number
    of roundings, so the honest float32 computation must pass the bar the kernel is held to (a bar it fails would be the wrong bar);
  * nearest resize, maxpool2: equal bit for bit (a selection);
  * roi_align, LayerNorm-partition, window attention, attractor: element-wise error at most 64 * 2^-24 of mag -- these evaluate sums of up to 144
    terms and exp in float32, tens of roundings;
  * log-binomial: at most 8 * 2^-24 * L of mag, L = 63 ln(1e4) / min t the largest logit of the case -- a float32 logit carries a few roundings of
    its own size (2.7e4 at t = min_temp = 0.0212), and a probability moves by the absolute error of its logit.  Loose on purpose: the GPU test takes the restatement's own error as
    the baseline; here only a different formula (error >= 1e-4) has to show.

Planted defects.  Each is applied to a float32 torch restatement on the CPU; the per-element bar rejects it, tests/f64_ref.py old_normwise_bar (the bar
of tests/op_checks.py) accepts it.  For the counted operations the bar is counted_bar; for the others it is baseline_bar against the honest
restatement's own error on the same operands."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import f64_image_ref as I
from tests.f64_ref import old_normwise_bar
from tests.fake_ops import ops as fake

f32 = np.float32


# ---------------- float32 restatements with planted defects ----------------
def _taps32(n_in, n_out, l1_from_next=None, bad_clamp=False):
    src = I.ac_scale(n_in, n_out) * np.arange(n_out, dtype=f32)
    i0 = np.floor(src).astype(np.int64)
    i1 = np.minimum(i0 + 1, n_in - 2 if bad_clamp else n_in - 1)
    l1 = src - i0.astype(f32)
    if l1_from_next is not None:
        nxt = I.ac_scale(n_in, n_out) * f32(l1_from_next + 1)
        l1[l1_from_next] = nxt - np.floor(nxt)
    return torch.from_numpy(i0), torch.from_numpy(i1), torch.from_numpy(l1)


def bilinear32(x, oh, ow, defect=None, arg=None):
    """csrc/imageops.hip bilerp in float32 torch: l0 (lx0 v00 + lx1 v01) + l1 (lx0 v10 + lx1 v11), l0 = 1 - l1.  Defects:
    'clamp': the horizontal tap i1 is clamped one column early (min(i0 + 1, W - 2)), so the last interval blends column W - 2 with itself;
    'l1_row': the vertical l1 of output row arg comes from scale * (arg + 1); 'chan': output channel arg scaled by 1 + 1e-4;
    'swap': the vertical weight of a pixel is the horizontal l1 of its column and the horizontal weight the vertical l1 of its row"""
    x = x.float()
    B, H, W, C = x.shape
    y0, y1, ly = _taps32(H, oh, l1_from_next=arg if defect == "l1_row" else None)
    x0, x1, lx = _taps32(W, ow, bad_clamp=defect == "clamp")
    wy, wx = ly[:, None].expand(oh, ow), lx[None, :].expand(oh, ow)
    if defect == "swap":
        wy, wx = wx, wy
    wy, wx = wy[None, :, :, None], wx[None, :, :, None]
    r0, r1 = x[:, y0], x[:, y1]
    out = (1 - wy) * ((1 - wx) * r0[:, :, x0] + wx * r0[:, :, x1]) + wy * ((1 - wx) * r1[:, :, x0] + wx * r1[:, :, x1])
    if defect == "chan":
        out[..., arg] *= 1 + 1e-4
    return out


def _run(fn, shape, dtype=torch.float32):
    y = torch.full(shape, float("nan"), dtype=dtype)
    fn(y)
    return y


def _rejected_but_old_bar_accepts(y_bad, ref, mag, k=None, base=None):
    if k is not None:
        rejected = not I.counted_bar(y_bad, ref, mag, k)[0]
    else:
        rejected = not I.baseline_bar(I.errors(y_bad, ref, mag), base)
    assert rejected, "the per-element bar accepts the defect"
    assert old_normwise_bar(y_bad, ref), "the old normwise bar rejects the defect too: it would have been caught before"


# ---------------- the honest float32 restatement passes the counted bars at every case of the GPU test ----------------
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("case", I.RESIZE_CASES, ids=lambda c: "x".join(map(str, c)))
def test_float32_resize_passes_the_counted_bar(case, dt):
    h, w, oh, ow, C = case
    x, add = I.features((2, h, w, C), h, dt), I.features((2, oh, ow, C), w + 1, dt)
    bf = dt == torch.bfloat16
    ref, mag = I.bilinear_ref(x, oh, ow)
    assert bool((mag == ref.abs()).all())                                         # positive inputs: no cancellation anywhere
    y = _run(lambda y: fake.resize(x, y), (2, oh, ow, C), dt)
    assert I.counted_bar(y, ref, mag, I.K_BILERP, bf)[0], I.counted_bar(y, ref, mag, I.K_BILERP, bf)
    if not bf:
        assert I.counted_bar(bilinear32(x, oh, ow), ref, mag, I.K_BILERP)[0]      # the restatement the defects are planted in
    ref, mag = I.bilinear_ref(x, oh, ow, add)
    y = _run(lambda y: fake.resize(x, y, add=add), (2, oh, ow, C), dt)
    assert I.counted_bar(y, ref, mag, I.K_BILERP_ADD, bf)[0]
    ref, mag = I.resize_concat_ref([x, add, x], oh, ow)
    buf = _run(lambda y: fake.resize_concat([x, add, x], y[..., 8:8 + 3 * C]), (2, oh, ow, 3 * C + 16), dt)
    assert I.counted_bar(buf[..., 8:8 + 3 * C], ref, mag, I.K_BILERP, bf)[0]
    assert torch.isnan(buf[..., :8]).all() and torch.isnan(buf[..., 8 + 3 * C:]).all()


def test_float32_planar_resizes_and_crop_pass_their_bars():
    for (h, w, oh, ow) in I.PLANE_CASES:
        x = I.features((h, w, 1), h)[..., 0]
        ref, mag = I.bilinear_plane_ref(x, oh, ow)
        assert I.counted_bar(_run(lambda y: fake.resize_bilinear_f32(x, y), (oh, ow)), ref, mag, I.K_BILERP)[0]
        assert torch.equal(_run(lambda y: fake.resize_nearest_f32(x, y), (oh, ow)), I.nearest_ref(x, oh, ow))
    img = I.features((96, 130, 3), 5).permute(2, 0, 1).contiguous()
    boxes = torch.tensor(I.CROP_BOXES, dtype=torch.int32)
    ref, mag = I.crop_resize_ref(img, boxes, 28, 42)
    assert I.counted_bar(_run(lambda y: fake.crop_resize(img, boxes, y), (len(I.CROP_BOXES), 3, 28, 42)), ref, mag, I.K_BILERP)[0]
    # the box of the output's size is a copy
    assert torch.equal(ref[5].float(), img[:, 30:58, 50:92])


def test_maxpool_reference_is_exact_and_drops_the_odd_edge():
    for dt in (torch.float32, torch.bfloat16):
        x = torch.randn(2, 49, 65, 32, generator=torch.Generator().manual_seed(1)).to(dt)
        want = I.maxpool2_ref(x)
        assert want.shape == (2, 24, 32, 32) and want.dtype == dt
        assert torch.equal(_run(lambda y: fake.maxpool2(x, y), (2, 24, 32, 32), dt), want)
        x2 = x.clone()
        x2[:, 48], x2[:, :, 64] = 1e3, 1e3                                        # the dropped row and column do not reach the output
        assert torch.equal(I.maxpool2_ref(x2), want)


def stitch_operands():
    g = torch.Generator().manual_seed(1)
    depth = torch.rand(6, 28, 42, generator=g) + 0.5
    mask = I.features((28, 42, 1), 2)[..., 0].contiguous()
    rawmask = I.features((40, 60, 1), 3)[..., 0].contiguous()
    small = torch.rand(20, 30, generator=g) + 0.5
    yx = torch.tensor([[0, 0], [0, 42], [28, 0], [28, 42]], dtype=torch.int32)
    return depth, mask, rawmask, small, yx


def test_float32_stitch_passes_the_counted_bars():
    depth, mask, rawmask, small, yx = stitch_operands()
    nan = lambda: torch.full((56, 84), float("nan"))
    pred, cnt, avg = nan(), nan(), nan()
    (rp, mp), rc = I.stitch_init_ref(pred, cnt, depth[:4], mask, yx)
    fake.stitch_init(pred, cnt, depth[:4], mask, yx)
    assert I.counted_bar(pred, rp, mp, I.K_STITCH_INIT)[0] and torch.equal(cnt.double(), rc)
    ra, ma = I.stitch_finish_ref(pred, cnt)
    fake.stitch_finish_init(avg, pred, cnt)
    assert I.counted_bar(avg, ra, ma, I.K_DIV)[0]
    for d, m, y0, x0 in ((depth[4], mask, 14, 21), (depth[5], mask, 28, 42), (small, rawmask, 9, 13)):
        (ra, ma), (rc, mc) = I.stitch_update_ref(avg, cnt, d, m, y0, x0)
        fake.stitch_update(avg, cnt, d, m, y0, x0)
        assert I.counted_bar(avg, ra, ma, I.K_STITCH_AVG)[0] and I.counted_bar(cnt, rc, mc, I.K_ADD)[0]


# ---------------- agreement of the other references with the restatements ----------------
def swin_operands(B, H, W, C, heads, dt, seed=0, v_features=False):
    g = torch.Generator().manual_seed(H * W + C + seed)
    Hp, Wp = I._pad12(H), I._pad12(W)
    nt = B * Hp * Wp
    x = (torch.randn(B, H, W, C, generator=g) * (0.5 + torch.rand(C, generator=g)) + torch.randn(C, generator=g)).to(dt)
    gam, bet = 1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    qkv = torch.randn(nt, 3 * C, generator=g)
    if v_features:
        qkv[:, 2 * C:] = I.features((nt, C), seed + 1)
    bt = torch.randn(529, heads, generator=g)                                     # unit standard deviation
    proj = torch.randn(nt, C, generator=g).to(dt)
    return x, gam, bet, qkv.to(dt), bt, proj, Hp, Wp, nt


@pytest.mark.parametrize("shift", [0, 6])
@pytest.mark.parametrize("case", I.SWIN_CASES, ids=lambda c: "x".join(map(str, c)))
def test_swin_references_agree_with_the_restatement(case, shift):
    B, H, W, C, heads = case
    x, gam, bet, qkv, bt, proj, Hp, Wp, nt = swin_operands(*case, torch.float32)
    ref, mag = I.swin_ln_partition_ref(x, gam, bet, 1e-5, shift)
    y = _run(lambda y: fake.swin_ln_partition(x, y, gam, bet, 1e-5, shift), (nt, C))
    assert I.errors(y, ref, mag)[0] <= 64 * I.U
    assert bool((y[mag == 0] == 0).all()) and int((mag == 0).sum()) >= (Hp * Wp - H * W) * B * C
    ref, mag = I.swin_window_attention_ref(qkv, bt, B, Hp, Wp, C, heads, shift)
    y = _run(lambda y: fake.swin_window_attention(qkv, y, bt, B, Hp, Wp, C, heads, shift), (nt, C))
    assert I.errors(y, ref, mag)[0] <= 64 * I.U
    ref, mag = I.swin_unpartition_add_ref(proj, x, shift)
    y = _run(lambda y: fake.swin_unpartition_add(proj, x, y, shift), (B, H, W, C))
    assert I.counted_bar(y, ref, mag, I.K_ADD)[0]


def roi_operands(h, w, C, dt=torch.float32, feat=True):
    g = torch.Generator().manual_seed(h)
    f = I.features((1, h, w, C), h, dt) if feat else torch.randn(1, h, w, C, generator=g).to(dt)
    return f, torch.tensor(I.ROIS)


@pytest.mark.parametrize("h,w,C", I.ROI_FEATS)
def test_roi_align_reference_agrees_with_the_restatement(h, w, C):
    for feat in (True, False):
        f, rois = roi_operands(h, w, C, feat=feat)
        ref, mag = I.roi_align_ref(f, rois, h, w, h / 112)
        y = _run(lambda y: fake.roi_align(f, rois, y, h / 112), (5, h, w, C))
        assert I.errors(y, ref, mag)[0] <= 64 * I.U
        assert bool((ref[4] == 0).all()) and bool((y[4] == 0).all())              # the RoI wholly outside samples nothing
        assert bool((ref[3, :, -1] != ref[2, :, -1]).any())


def test_roi_align_multi_sample_and_depth_agree():
    f = I.features((2, 16, 16, 8), 3)
    r2 = torch.tensor([[1, 0.0, 0.0, 16.0, 16.0], [0, 2.0, 3.0, 14.0, 12.0]])
    ref, mag = I.roi_align_ref(f, r2, 4, 5, 1.0)
    y = _run(lambda y: fake.roi_align(f, r2, y, 1.0), (2, 4, 5, 8))
    assert I.errors(y, ref, mag)[0] <= 64 * I.U
    d = torch.rand(1, 1, 112, 154, generator=torch.Generator().manual_seed(9))
    ref, mag = I.roi_align_depth_ref(d, torch.tensor(I.ROIS), 112, 154, 1.0)
    y = _run(lambda y: fake.roi_align_depth(d, torch.tensor(I.ROIS), y, 1.0), (5, 1, 112, 154))
    assert I.errors(y, ref, mag)[0] <= 64 * I.U


def attractor_operands(n_attr, hp, wp, h, w, a_level=None, stride=1):
    g = torch.Generator().manual_seed(n_attr * 100 + h)
    na = ((n_attr - 1) * stride + 1 + 3) // 4 * 4
    if a_level is None:
        A = F.softplus(torch.randn(2, h, w, na, generator=g))
        bp = F.softplus(torch.randn(2, hp, wp, 64, generator=g))
    else:                                   # attractors a_level above the centres, both with low-amplitude detail
        A = a_level + I.features((2, h, w, na), 7)
        bp = I.features((2, hp, wp, 64), 8)
    return A, bp


BINS = [(16, (4, 6, 8, 11)), (8, (8, 11, 16, 22)), (1, (32, 44, 64, 88))]
VARIANTS = [dict(a_stride=2, a_eps=1e-3), dict(a_stride=2, a_eps=1e-3, attractor_type="exp", kind="sum"), dict(attractor_type="exp"), dict(kind="sum")]


def test_attractor_reference_agrees_with_the_restatement():
    for n_attr, (hp, wp, h, w) in BINS:
        A, bp = attractor_operands(n_attr, hp, wp, h, w)
        ref, mag = I.attractor_ref(A, n_attr, bp, h, w)
        assert I.errors(_run(lambda y: fake.attractor(A, n_attr, bp, y), (2, h, w, 64)), ref, mag)[0] <= 64 * I.U
    for kw in VARIANTS:
        A, bp = attractor_operands(16, 8, 11, 16, 22, stride=kw.get("a_stride", 1))
        ref, mag = I.attractor_ref(A, 16, bp, 16, 22, **kw)
        assert I.errors(_run(lambda y: fake.attractor(A, 16, bp, y, **kw), (2, 16, 22, 64)), ref, mag)[0] <= 64 * I.U


def logbinom_operands(ends=False, flat_centres=False):
    g = torch.Generator().manual_seed(5)
    pt = F.softplus(torch.randn(2, 56, 77, 4, generator=g) + torch.tensor([0, 0, -4.0, 1.0]))
    if ends:                                # t0 / (t0 + t1) -> 0 in the left half (t = min_temp), -> 1 in the right half (t = max_temp)
        pt[:, :, :38, 2], pt[:, :, :38, 3] = 0.0, 30.0
        pt[:, :, 38:, 2], pt[:, :, 38:, 3] = 30.0, 0.0
    cen = 1.0 + 2.0 ** -16 * torch.randn(2, 32, 44, 64, generator=g) if flat_centres else F.softplus(torch.randn(2, 32, 44, 64, generator=g))
    return pt, cen


@pytest.mark.parametrize("ends", [False, True])
def test_logbinom_reference_agrees_with_the_restatement(ends):
    pt, cen = logbinom_operands(ends)
    ref, mag = I.logbinom_depth_ref(pt, cen, 56, 77, 0.0212, 50.0)
    y = _run(lambda y: fake.logbinom_depth(pt, cen, y, 0.0212, 50.0), (2, 56, 77))
    q = pt.double()[..., 2:4] + 1e-4
    t = q[..., 0] / q.sum(-1)
    logit = 63 * math.log(1e4) / float(((50.0 - 0.0212) * t + 0.0212).min())      # the largest |logit| / t of the case (p, 1 - p >= 1e-4)
    assert I.errors(y, ref, mag)[0] <= 8 * I.U * logit
    if ends:                                # the case really reaches both ends of the temperature range
        assert float(t.min()) < 1e-5 and float(t.max()) > 1 - 1e-5


# ---------------- planted defects ----------------
@pytest.mark.parametrize("defect,arg,case", [("clamp", None, (14, 19, 28, 37, 64)), ("l1_row", 13, (14, 19, 28, 37, 64)), ("chan", 5, (14, 19, 28, 37, 64)),
                                             ("swap", None, (8, 11, 9, 11, 64))], ids=["clamp", "l1_row", "chan", "swap"])
def test_resize_defects(defect, arg, case):
    h, w, oh, ow, C = case
    x = I.features((2, h, w, C), h)
    ref, mag = I.bilinear_ref(x, oh, ow)
    assert I.counted_bar(bilinear32(x, oh, ow), ref, mag, I.K_BILERP)[0]
    _rejected_but_old_bar_accepts(bilinear32(x, oh, ow, defect, arg), ref, mag, k=I.K_BILERP)


def test_roi_sample_offset_defect():
    f, rois = roi_operands(28, 37, 64)
    rois = rois[:4]
    ref, mag = I.roi_align_ref(f, rois, 28, 37, 0.25)
    base = I.errors(_run(lambda y: fake.roi_align(f, rois, y, 0.25), (4, 28, 37, 64)), ref, mag)
    bad = rois.clone()
    bad[2, 1:] += 0.5 / 0.25                                                       # half a feature pixel, one RoI
    _rejected_but_old_bar_accepts(_run(lambda y: fake.roi_align(f, bad, y, 0.25), (4, 28, 37, 64)), ref, mag, base=base)


def _attention32(qkv, bt, B, Hp, Wp, C, heads, shift, defect=None):
    """fake_ops.swin_window_attention with 'mask_last' (no shift mask in the last window) or 'transpose' (relative-position index transposed)"""
    from oracle.pf_oracle import swin_shift_mask
    nW, hd = qkv.shape[0] // 144, C // heads
    q, k, v = qkv.float().view(nW, 144, 3, heads, hd).permute(2, 0, 3, 1, 4)
    attn = (q * hd ** -0.5) @ k.transpose(-2, -1)
    idx = I.relative_position_index()
    idx = idx.t() if defect == "transpose" else idx
    attn = attn + bt[idx.reshape(-1)].view(144, 144, heads).permute(2, 0, 1).unsqueeze(0)
    if shift > 0:
        mask = swin_shift_mask(Hp, Wp, 12, shift, "cpu").clone()
        if defect == "mask_last":
            mask[-1] = 0
        attn = (attn.view(B, nW // B, heads, 144, 144) + mask.unsqueeze(1).unsqueeze(0)).view(-1, heads, 144, 144)
    return (attn.softmax(-1) @ v).transpose(1, 2).reshape(nW * 144, C)


@pytest.mark.parametrize("defect", ["mask_last", "transpose"])
def test_window_attention_defects(defect):
    case = (1, 12, 24, 64, 16)
    B, H, W, C, heads = case
    x, gam, bet, qkv, bt, proj, Hp, Wp, nt = swin_operands(*case, torch.float32, v_features=True)
    ref, mag = I.swin_window_attention_ref(qkv, bt, B, Hp, Wp, C, heads, 6)
    honest = _attention32(qkv, bt, B, Hp, Wp, C, heads, 6)
    assert torch.equal(honest, _run(lambda y: fake.swin_window_attention(qkv, y, bt, B, Hp, Wp, C, heads, 6), (nt, C)))
    _rejected_but_old_bar_accepts(_attention32(qkv, bt, B, Hp, Wp, C, heads, 6, defect), ref, mag, base=I.errors(honest, ref, mag))


def test_swin_roll_sign_defect():
    """+shift instead of -shift in the partition; a map without padding (a padded one moves zeros onto real tokens, which the old bar sees too)"""
    B, H, W, C = 1, 12, 24, 64
    g = torch.Generator().manual_seed(4)
    x = I.features((B, H, W, C), 11)
    gam, bet = 1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    ref, mag = I.swin_ln_partition_ref(x, gam, bet, 1e-5, 6)
    base = I.errors(_run(lambda y: fake.swin_ln_partition(x, y, gam, bet, 1e-5, 6), (B * H * W, C)), ref, mag)
    v = torch.roll(F.layer_norm(x, (C,), gam, bet, 1e-5), shifts=(6, 6), dims=(1, 2))
    bad = v.view(B, H // 12, 12, W // 12, 12, C).permute(0, 1, 3, 2, 4, 5).reshape(-1, C)
    assert not torch.equal(bad.double(), ref.float().double())
    _rejected_but_old_bar_accepts(bad, ref, mag, base=base)


def test_attractor_defects():
    # a_eps dropped: attractors 0.3 above the centres (|d'(0.3)| = 0.03: the output moves by 3e-5)
    A, bp = attractor_operands(16, 8, 11, 16, 22, a_level=0.3, stride=2)
    kw = dict(a_stride=2, a_eps=1e-3)
    ref, mag = I.attractor_ref(A, 16, bp, 16, 22, **kw)
    base = I.errors(_run(lambda y: fake.attractor(A, 16, bp, y, **kw), (2, 16, 22, 64)), ref, mag)
    _rejected_but_old_bar_accepts(_run(lambda y: fake.attractor(A, 16, bp, y, a_stride=2, a_eps=0.0), (2, 16, 22, 64)), ref, mag, base=base)
    # the mean over n_attr + 1: attractors 2 above the centres (d = 2 / 1201: the output moves by 1e-4)
    A, bp = attractor_operands(16, 8, 11, 16, 22, a_level=2.0)
    ref, mag = I.attractor_ref(A, 16, bp, 16, 22)
    base = I.errors(_run(lambda y: fake.attractor(A, 16, bp, y), (2, 16, 22, 64)), ref, mag)
    c = F.interpolate(bp.permute(0, 3, 1, 2), size=(16, 22), mode="bilinear", align_corners=True)
    dx = A[..., :16].permute(0, 3, 1, 2).unsqueeze(2) - c.unsqueeze(1)
    bad = (c + (dx / (1 + 300.0 * dx.pow(2))).sum(1) / 17).permute(0, 2, 3, 1)
    _rejected_but_old_bar_accepts(bad, ref, mag, base=base)


def test_logbinom_swapped_temperatures_defect():
    pt, cen = logbinom_operands(flat_centres=True)
    ref, mag = I.logbinom_depth_ref(pt, cen, 56, 77, 0.0212, 50.0)
    base = I.errors(_run(lambda y: fake.logbinom_depth(pt, cen, y, 0.0212, 50.0), (2, 56, 77)), ref, mag)
    _rejected_but_old_bar_accepts(_run(lambda y: fake.logbinom_depth(pt, cen, y, 50.0, 0.0212), (2, 56, 77)), ref, mag, base=base)


def test_stitch_mask_offset_defect():
    depth, mask, rawmask, small, yx = stitch_operands()
    avg, cnt = torch.rand(56, 84, generator=torch.Generator().manual_seed(7)) + 0.5, I.features((56, 84, 1), 8)[..., 0].contiguous()
    (ra, ma), (rc, mc) = I.stitch_update_ref(avg, cnt, depth[4], mask, 14, 21)
    a, c = avg.clone(), cnt.clone()
    fake.stitch_update(a, c, depth[4], mask, 14, 21)
    assert I.counted_bar(a, ra, ma, I.K_STITCH_AVG)[0] and I.counted_bar(c, rc, mc, I.K_ADD)[0]
    a, c = avg.clone(), cnt.clone()
    fake.stitch_update(a, c, depth[4], torch.roll(mask, -1, 1), 14, 21)           # mask[y, x + 1] for the map element (y0 + y, x0 + x)
    _rejected_but_old_bar_accepts(a, ra, ma, k=I.K_STITCH_AVG)
    _rejected_but_old_bar_accepts(c, rc, mc, k=I.K_ADD)
