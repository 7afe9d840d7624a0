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
restatement's own error on the same operands.

The fused metric-bins tail, the bin centres, the copies and the mixed-dtype resize (tests/test_tail_grade_gpu.py), at every shape, operand kind and
grid of that test: fake_ops.bins_tail agrees with bins_tail_ref, and the float32 evaluation in the KERNEL's order (tail32: the K groups of the MFMA
operand, the hidden channels and the bins split over four lane groups, the xor-shuffle sums) meets baseline_bar against it -- the bar the kernel is
held to can be met.  Ten defects are planted in tail32 and rejected (test_tail_defects; OP_CHECKS_ACCEPTS records that tests/op_checks.py's own
operands and 1e-4 accept four of them); one listed change, (64 - k) for (63 - k), shifts every logit of a pixel alike and leaves the softmax as it is
(test_64_minus_k_is_no_defect_of_the_function), and so does a clip moved in front of the sort alone.  One defect each for seed_bin_centers (edge sum
from 0: accepted by op_checks.bins_ops, which divides by 80), bounded_bin_centers and the bf16 copies (truncation: accepted by misc_ops' 1e-2)."""
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
def _taps32(n_in, n_out, l1_from_next=None, bad_clamp=False, scale_from=None):
    """scale_from: the scale is that of a source of scale_from elements (another map's grid); the taps are then clamped into this one (the kernel
    would read outside it)"""
    src = I.ac_scale(n_in if scale_from is None else scale_from, n_out) * np.arange(n_out, dtype=f32)
    i0 = np.floor(src).astype(np.int64)
    l1 = src - i0.astype(f32)
    i0 = np.minimum(i0, n_in - 1)
    i1 = np.minimum(i0 + 1, max(n_in - 2, 0) if bad_clamp else n_in - 1)
    if l1_from_next is not None:
        nxt = I.ac_scale(n_in, n_out) * f32(l1_from_next + 1)
        l1[l1_from_next] = nxt - np.floor(nxt)
    return torch.from_numpy(i0), torch.from_numpy(i1), torch.from_numpy(l1)


def bilinear32(x, oh, ow, defect=None, arg=None):
    """csrc/imageops.hip bilerp in float32 torch: l0 (lx0 v00 + lx1 v01) + l1 (lx0 v10 + lx1 v11), l0 = 1 - l1.  Defects:
    'clamp': the horizontal tap i1 is clamped one column early (min(i0 + 1, W - 2)), so the last interval blends column W - 2 with itself;
    'l1_row': the vertical l1 of output row arg comes from scale * (arg + 1); 'chan': output channel arg scaled by 1 + 1e-4;
    'swap': the vertical weight of a pixel is the horizontal l1 of its column and the horizontal weight the vertical l1 of its row;
    'clamp_row': the vertical tap i1 is clamped one row early; 'grid': the scales are those of a source of arg = (rows, columns)"""
    x = x.float()
    B, H, W, C = x.shape
    gy, gx = arg if defect == "grid" else (None, None)
    y0, y1, ly = _taps32(H, oh, l1_from_next=arg if defect == "l1_row" else None, bad_clamp=defect == "clamp_row", scale_from=gy)
    x0, x1, lx = _taps32(W, ow, bad_clamp=defect == "clamp", scale_from=gx)
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


# ---------------- the fused metric-bins tail, the bin centres and the copies (tests/test_tail_grade_gpu.py) ----------------
NAN = float("nan")
OLD_TAIL_TOL = 1e-4                 # tests/op_checks.py bins_tail


def op_checks_bar(y, want, tol=OLD_TAIL_TOL):
    """tests/op_checks.py _err: max |y - want| / max(1, max |want|) <= tol against the float32 torch restatement"""
    y, want = y.double(), want.double()
    return bool(torch.isfinite(y).all()) and float((y - want).abs().max()) / max(1.0, float(want.abs().max())) <= tol


def fake_tail(o, H, W, tw=None):
    """tests/fake_ops.py bins_tail (resize, two 1x1 convolutions, log-binomial expectation in float32 torch) on the operands -> depth [B, H, W]"""
    tw = tw or I.tail_pack(o)
    depth = torch.full(o["last"].shape[:3], NAN)
    fake.bins_tail(I.tail_clb(o), o["emb"], tw, o["centers"], depth, I.MIN_TEMP, I.MAX_TEMP)
    return depth


TAIL_DEFECTS = ("rel_all_groups", "cen_emb_scales", "omk_64", "omk_lane_local", "logc_eps", "x_10bit", "emb_clamp_row", "gelu_tanh", "b2_early",
                "pt_eps", "max_one_group")


def tail32(o, H, W, defect=None, wide=True):
    """csrc/imageops.hip bins_tail_kernel in float32 torch, in the kernel's order: the operand of K group q, slot e holds channels 16 q + 4 g + e of
    the four lane groups g (one 16x16x4 MFMA step, accumulated over (q, e)); the embedding blended with the resize kernels' expression; lane group
    g owns hidden channels 16 f + 4 g + e and bins 16 g + j; partial sums per group, then (s0 + s1) + (s2 + s3) as the two xor-shuffles form them.
    The order of tests/test_bins_tail_model_cpu.py, vectorised over the pixels and in float32.  Defects (the issue's list):
      rel_all_groups  lane groups 2, 3 load the rel K group too: they read the 8 channels after rel, which meet zero weights.  wide: those are NaN
                      (the CLB buffer is a channel view of a wider NaN-filled one); not wide: the buffer is contiguous and they are the first 8
                      channels of the next pixel (of nothing after the last pixel: zeros here, an out-of-bounds read in the kernel)
      cen_emb_scales  the centres' taps from the embedding's scales she, swe
      omk_64          (64 - k) lq for (63 - k) lq.  Adds lq / t to every logit: the softmax does not change.  NOT a defect of the function (see the test)
      omk_lane_local  (63 - j) lq with the lane's own bin index j = k mod 16: a different shift per lane group
      logc_eps        log(n - k) for log(n - k + 1e-7) in the Stirling term: 0 log 0 at k = 63
      x_10bit         the operand x cut to 10 mantissa bits before the product (the xf32 MFMA)
      emb_clamp_row   the embedding's lower tap clamped one row early
      gelu_tanh       the tanh form of GELU
      b2_early        b2 added before the cross-group sum (four times)
      pt_eps          no + 1e-4 on p0, p1, t0, t1
      max_one_group   every lane group subtracts the maximum of its own 16 bins"""
    assert defect is None or defect in TAIL_DEFECTS
    last, rel, emb, cen = o["last"], o["rel"], o["emb"], o["centers"]
    B = last.shape[0]
    P = B * H * W
    nq = 10 if rel is None else 11
    X = torch.zeros(P, 16 * nq)
    X[:, :32] = last.reshape(P, 32)
    X[:, 32:160] = bilinear32(emb, H, W, "clamp_row" if defect == "emb_clamp_row" else None).reshape(P, 128)
    if rel is not None:
        X[:, 160:168] = rel.reshape(P, 8)
        if defect == "rel_all_groups":
            X[:, 168:176] = NAN
            if not wide:
                X[:-1, 168:176], X[-1, 168:176] = X[1:, :8], 0.0
    if defect == "x_10bit":
        X = (X.view(torch.int32) & -8192).view(torch.float32)
    Wp = torch.zeros(80, 16 * nq)
    Wp[:, :o["w0"].shape[1]] = o["w0"]
    acc = torch.zeros(P, 80)
    g4 = 4 * torch.arange(4)
    for q in range(nq):
        for e in range(4):
            idx = 16 * q + g4 + e
            acc = acc + X[:, idx] @ Wp[:, idx].t()
    v = acc + o["b0"]
    t = F.gelu(v, approximate="tanh") if defect == "gelu_tanh" else F.gelu(v)
    part = torch.zeros(P, 4, 4)                                                  # [pixel, lane group, output]
    for f in range(5):
        for e in range(4):
            ch = 16 * f + g4 + e
            part = part + t[:, ch, None] * o["w2"][:, ch].t()[None]
    if defect == "b2_early":
        part = part + o["b2"]
    o4 = (part[:, 0] + part[:, 1]) + (part[:, 2] + part[:, 3])
    if defect != "b2_early":
        o4 = o4 + o["b2"]
    o4 = torch.where(o4 > 20.0, o4, torch.log1p(torch.exp(torch.clamp(o4, max=20.0))))
    q4 = o4 if defect == "pt_eps" else o4 + 1e-4
    p = q4[:, 0] / (q4[:, 0] + q4[:, 1])
    tt = q4[:, 2] / (q4[:, 2] + q4[:, 3])
    tt = ((I.MAX_TEMP - I.MIN_TEMP) * tt + I.MIN_TEMP)[:, None]
    om = torch.clamp(1 - p, 1e-4, 1.0)[:, None]
    p = torch.clamp(p, 1e-4, 1.0)[:, None]
    eps = torch.tensor(1e-7)
    k = torch.arange(64, dtype=torch.float32)
    n_, k_ = 63.0 + eps, k + eps
    logc = n_ * torch.log(n_) - k_ * torch.log(k_) - (n_ - k_) * torch.log(n_ - k_ if defect == "logc_eps" else n_ - k_ + eps)
    omk = {"omk_64": 64.0 - k, "omk_lane_local": 63.0 - k % 16}.get(defect, 63.0 - k)
    yk = ((logc + k * torch.log(p) + omk * torch.log(om)) / tt).view(P, 4, 16)
    mx = yk.amax(-1, keepdim=True)
    if defect != "max_one_group":
        mx = mx.amax(1, keepdim=True)
    pe = torch.exp(yk - mx)
    c = bilinear32(cen, H, W, "grid" if defect == "cen_emb_scales" else None, emb.shape[1:3]).reshape(P, 4, 16)
    num, den = torch.zeros(P, 4), torch.zeros(P, 4)
    for j in range(16):
        num = num + pe[..., j] * c[..., j]
        den = den + pe[..., j]
    num = (num[:, 0] + num[:, 1]) + (num[:, 2] + num[:, 3])
    den = (den[:, 0] + den[:, 1]) + (den[:, 2] + den[:, 3])
    return (num / den).view(B, H, W)


def _largest_logit(o, H, W):
    """63 ln(1e4) / min t of the case, t from the float64 tail: the size of the largest logit a float32 evaluation forms"""
    e, _ = I.bilinear_ref(o["emb"], H, W)
    x = torch.cat([o["last"].double(), e] + ([] if o["rel"] is None else [o["rel"].double()]), -1)
    h = F.gelu(x @ o["w0"].double().t() + o["b0"].double())
    q = F.softplus(h @ o["w2"].double().t() + o["b2"].double())[..., 2:4] + 1e-4
    t = (I.MAX_TEMP - I.MIN_TEMP) * q[..., 0] / q.sum(-1) + I.MIN_TEMP
    return 63 * math.log(1e4) / float(t.min()), float(t.min()), float(t.max())


@pytest.mark.parametrize("case", I.TAIL_CASES, ids=[c[0] for c in I.TAIL_CASES])
def test_float32_tail_meets_the_bar_of_the_gpu_test(case):
    """at every shape, kind and grid of the GPU test: fake_ops.bins_tail agrees with bins_tail_ref to 8 * 2^-24 * L of mag (L the largest logit, as for
    the log-binomial alone, plus the 64 roundings of the two layers), and the float32 evaluation in the KERNEL's order (tail32) passes the bar the
    kernel is held to -- baseline_bar against fake_ops.bins_tail on the same operands.  The kinds reach what they are named for."""
    name, kind, ctot, (B, H, W), eg, cg = case
    o = I.tail_operands(kind, ctot, B, H, W, eg, cg)
    ref, mag = I.tail_ref(o, H, W)
    assert bool(torch.isfinite(ref).all()) and bool((mag >= ref.abs() - 1e-12).all())
    base = I.errors(fake_tail(o, H, W), ref, mag)
    logit, tmin, tmax = _largest_logit(o, H, W)
    assert base[0] <= (8 * logit + 64) * I.U, (name, base, logit)
    e = I.errors(tail32(o, H, W), ref, mag)
    print(f"{name:40s} kernel-order f32 elem {e[0]:.2e} norm {e[1]:.2e} | fake_ops elem {base[0]:.2e} norm {base[1]:.2e}")
    assert I.baseline_bar(e, base), (name, e, base)
    if kind == "t_low":
        assert tmax < I.MIN_TEMP * 1.02
    if kind == "t_high":
        assert tmin > I.MAX_TEMP * 0.999
    if kind == "random":
        assert not bool((o["centers"][..., 1:] >= o["centers"][..., :-1]).all())


def test_tail_kinds_reach_the_clamps_and_the_linear_softplus():
    H, W = 37, 50
    for ctot in (168, 160):
        o = I.tail_operands("p_ends", ctot, 2, H, W)
        e, _ = I.bilinear_ref(o["emb"], H, W)
        x = torch.cat([o["last"].double(), e] + ([] if o["rel"] is None else [o["rel"].double()]), -1)
        pre = F.gelu(x @ o["w0"].double().t() + o["b0"].double()) @ o["w2"].double().t() + o["b2"].double()
        q = F.softplus(pre)[..., :2] + 1e-4
        p = (q[..., 0] / q.sum(-1)).view(-1)
        half = p.numel() // 2
        assert float((1 - p[:half]).max()) < 1e-4 and float(p[half:].max()) < 1e-4          # both clamps, in halves of the map
        o = I.tail_operands("softplus_linear", ctot, 2, H, W)
        e, _ = I.bilinear_ref(o["emb"], H, W)
        x = torch.cat([o["last"].double(), e] + ([] if o["rel"] is None else [o["rel"].double()]), -1)
        pre = F.gelu(x @ o["w0"].double().t() + o["b0"].double()) @ o["w2"].double().t() + o["b2"].double()
        above = (pre[..., :2] > 20).double().mean()
        assert 0.2 < float(above) < 0.9, float(above)


# defect -> (kind, ctot, emb grid, centres grid) of the operands it is planted in, at 2 x 37 x 50
_G, _C = I.TAIL_EMB_GRID, I.TAIL_CEN_GRID
TAIL_DEFECT_CASES = {
    "rel_all_groups": ("random", 168, _G, _C), "cen_emb_scales": ("sorted", 168, _G, _C), "omk_lane_local": ("random", 168, _G, _C),
    "logc_eps": ("random", 168, _G, _C), "x_10bit": ("random", 168, _G, _C), "emb_clamp_row": ("random", 168, _G, _C),
    "gelu_tanh": ("random", 160, _G, _C), "b2_early": ("random", 168, _G, _C), "pt_eps": ("random", 160, _G, _C),
    "max_one_group": ("random", 168, _G, _C)}
# what was found: does tests/op_checks.py bins_tail (its operands, its 1e-4) accept the defect?  Four of ten: the extra rel loads (finite values on
# zero weights in its contiguous buffer), the centres on the embedding's scales (its two grids are the same), tanh-GELU and the dropped 1e-4
OP_CHECKS_ACCEPTS = {"rel_all_groups": True, "cen_emb_scales": True, "omk_lane_local": False, "logc_eps": False, "x_10bit": False,
                     "emb_clamp_row": False, "gelu_tanh": True, "b2_early": False, "pt_eps": True, "max_one_group": False}


def _op_checks_verdict(defect):
    """does tests/op_checks.py bins_tail accept the defect?  Its operands: 2 x 37 x 50, sorted centres on the embedding's grid, mid-range temperatures;
    its bar: 1e-4 normwise against the float32 torch restatement"""
    o = I.tail_operands("sorted", TAIL_DEFECT_CASES[defect][1], 2, 37, 50, _G, _G)
    return op_checks_bar(tail32(o, 37, 50, defect, wide=False), fake_tail(o, 37, 50))


@pytest.mark.parametrize("defect", list(TAIL_DEFECT_CASES))
def test_tail_defects(defect):
    """every planted defect fails baseline_bar (or leaves a non-finite output, which errors() reports as inf) on operands of the GPU test; printed
    and held to OP_CHECKS_ACCEPTS: whether op_checks' own operands and 1e-4 bar accept it.  rel_all_groups is planted with the CLB buffer as a
    channel view of a wider NaN-filled one (a case of the GPU test); in a contiguous buffer it changes no output at all."""
    kind, ctot, eg, cg = TAIL_DEFECT_CASES[defect]
    H, W = 37, 50
    o = I.tail_operands(kind, ctot, 2, H, W, eg, cg)
    ref, mag = I.tail_ref(o, H, W)
    base = I.errors(fake_tail(o, H, W), ref, mag)
    assert I.baseline_bar(I.errors(tail32(o, H, W), ref, mag), base)
    bad = tail32(o, H, W, defect)
    e = I.errors(bad, ref, mag)
    old = _op_checks_verdict(defect)
    print(f"{defect:16s} elem {e[0]:.2e} norm {e[1]:.2e} | baseline elem {base[0]:.2e} norm {base[1]:.2e} | finite {bool(torch.isfinite(bad).all())}"
          f" | op_checks 1e-4 {'ACCEPTS' if old else 'rejects'}")
    assert not I.baseline_bar(e, base), "the per-element bar accepts the defect"
    assert old == OP_CHECKS_ACCEPTS[defect], "the recorded verdict of op_checks' bar is out of date"
    if defect == "rel_all_groups":
        assert torch.equal(tail32(o, H, W, defect, wide=False), tail32(o, H, W))


def test_64_minus_k_is_no_defect_of_the_function():
    """(64 - k) lq for (63 - k) lq adds lq / t to every logit of a pixel, and a softmax does not change under a common shift: the planted change
    leaves the function as it is, in float64 exactly and in float32 within the baseline.  No bar on outputs can reject it (none should); the
    neighbouring defect that IS one -- the lane-local (63 - j), a different shift per lane group -- is in test_tail_defects."""
    H, W = 37, 50
    for kind in ("random", "t_low", "p_ends"):
        o = I.tail_operands(kind, 168, 2, H, W)
        ref, mag = I.tail_ref(o, H, W)
        base = I.errors(fake_tail(o, H, W), ref, mag)
        e = I.errors(tail32(o, H, W, "omk_64"), ref, mag)
        print(f"omk_64 {kind:8s} elem {e[0]:.2e} norm {e[1]:.2e} | baseline elem {base[0]:.2e} norm {base[1]:.2e}")
        assert I.baseline_bar(e, base)
    yk = torch.randn(5, 64, dtype=torch.float64)
    cen = torch.rand(64, dtype=torch.float64)
    assert torch.allclose((yk.softmax(-1) * cen).sum(-1), ((yk - 434.0).softmax(-1) * cen).sum(-1), rtol=1e-12, atol=0)


# ---- bin centres ----
SEED_SHAPES = [((2, 9, 13), 64, 64), ((2, 9, 13), 16, 16), ((2, 9, 13), 16, 24), ((1, 1, 1), 64, 72), ((1, 1, 1), 16, 16)]      # pixels, n_bins, x_ld
HEAD_RANGE = (1e-3, 80.0)


def seed32(x, n_bins, lo, hi, bounded, normalize, defect=False):
    """csrc/imageops.hip seed_bin_centers_kernel in float32 torch, channels walked in order; defect: the edge sum starts at 0 instead of lo"""
    lo, hi = torch.tensor(lo, dtype=torch.float32), torch.tensor(hi, dtype=torch.float32)
    rng = hi - lo
    c = x[..., :n_bins].float()
    if bounded:
        s = torch.zeros_like(c[..., 0])
        for k in range(n_bins):
            s = s + (c[..., k] + 1e-3)
        e0 = torch.zeros_like(s) if defect else torch.zeros_like(s) + lo
        out = []
        for k in range(n_bins):
            e1 = e0 + rng * ((c[..., k] + 1e-3) / s)
            out.append(0.5 * (e0 + e1))
            e0 = e1
        c = torch.stack(out, -1)
    return (c - lo) / rng if normalize else c


def seed_baseline(x, nb, lo, hi, bounded, normalize, ref, mag, y_fake):
    """the baseline of the bounded seed centres: errors() of fake_ops or of the kernel-order float32 evaluation on the CPU, whichever is larger"""
    b, m = I.errors(y_fake, ref, mag), I.errors(seed32(x.cpu(), nb, lo, hi, bounded, normalize), ref, mag)
    return max(b[0], m[0]), max(b[1], m[1])


def _seed_case(shape, nb, ld, lo, hi, bounded, normalize):
    x = I.seed_operands(shape, nb, ld)
    ref, mag = I.seed_bin_centers_ref(x, nb, lo, hi, bounded, normalize)
    y = _run(lambda y: fake.seed_bin_centers(x, y, lo, hi, bounded, normalize), (*shape, nb))
    return x, ref, mag, y


@pytest.mark.parametrize("shape,nb,ld", SEED_SHAPES)
def test_float32_seed_bin_centers_meet_their_bars(shape, nb, ld):
    """the bounded combinations of the engine at the head's range: fake_ops and the kernel-order float32 evaluation (seed32) both within the first-order
    bound of the kernel's order, (2 nb + 6) 2^-24 mag -- nb - 1 for the sum of Bn walked in order, 2 for quotient and product, nb for the running edge
    sum, 1 for the centre, 2 for the normalisation.  torch sums the contiguous axis in vector lanes and is up to 5 times closer than the in-order walk
    (1.2e-6 against 2.8e-7 at 64 bins), so seed32 misses twice fake_ops' error: the baseline of the GPU test is the larger of the two (seed_baseline).
    Unbounded + normalize at ranges that are float32 numbers: both within 2 roundings; unbounded alone: a copy"""
    for bounded, normalize in ((True, True), (True, False)):
        x, ref, mag, y = _seed_case(shape, nb, ld, *HEAD_RANGE, bounded, normalize)
        base, model = I.errors(y, ref, mag), I.errors(seed32(x, nb, *HEAD_RANGE, bounded, normalize), ref, mag)
        print(f"seed_bin_centers {shape} nb {nb} bounded normalize={normalize}: fake_ops elem {base[0]:.2e} | kernel order elem {model[0]:.2e}")
        assert max(base[0], model[0]) <= (2 * nb + 6) * I.U, (base, model)
        assert I.baseline_bar(model, seed_baseline(x, nb, *HEAD_RANGE, bounded, normalize, ref, mag, y))
        assert bool((ref[..., 1:] >= ref[..., :-1]).all())                        # bounded centres ascend
    for lo, hi in I.EXACT_RANGES:
        assert float(f32(hi) - f32(lo)) == float(f32(hi)) - float(f32(lo))
        x, ref, mag, y = _seed_case(shape, nb, ld, lo, hi, False, True)
        assert I.counted_bar(y, ref, mag, I.K_SEED_NORM)[0], I.counted_bar(y, ref, mag, I.K_SEED_NORM)
        assert I.counted_bar(seed32(x, nb, lo, hi, False, True), ref, mag, I.K_SEED_NORM)[0]
    x, ref, mag, y = _seed_case(shape, nb, ld, *HEAD_RANGE, False, False)
    assert torch.equal(y, x[..., :nb]) and torch.equal(ref, x[..., :nb].double())


def test_seed_edge_sum_started_at_zero_defect():
    """lo = 1e-3 on centres up to 80: 1.2e-5 of the largest, 0.5 of the first centre"""
    shape, nb = (2, 9, 13), 64
    x, ref, mag, y = _seed_case(shape, nb, nb, *HEAD_RANGE, True, False)
    base = seed_baseline(x, nb, *HEAD_RANGE, True, False, ref, mag, y)
    bad = seed32(x, nb, *HEAD_RANGE, True, False, defect=True)
    assert not I.baseline_bar(I.errors(bad, ref, mag), base)
    old = float((bad - y).abs().max()) / max(1.0, float(y.abs().max())) / 80.0 <= 1e-4       # op_checks.bins_ops divides by 80
    print(f"seed edge sum from 0: elem {I.errors(bad, ref, mag)[0]:.2e} | baseline {base[0]:.2e} | op_checks 1e-4 {'ACCEPTS' if old else 'rejects'}")
    assert old


BOUNDED_CASES = [(npix, nb) for nb in (64, 16, 63, 1) for npix in (1, 5)]


@pytest.mark.parametrize("npix,nb", BOUNDED_CASES)
def test_float32_bounded_bin_centers_pass_the_counted_bar(npix, nb):
    for lo, hi in I.EXACT_RANGES:
        b = I.bounded_operands(npix, nb)
        ref, mag = I.bounded_bin_centers_ref(b, lo, hi)
        y = _run(lambda y: fake.bounded_bin_centers(b, y, lo, hi), tuple(b.shape))
        assert I.counted_bar(y, ref, mag, I.K_BOUNDED)[0], I.counted_bar(y, ref, mag, I.K_BOUNDED)
        assert bool((ref[..., 1:] >= ref[..., :-1]).all()) and float(ref.min()) >= float(f32(lo)) and float(ref.max()) <= float(f32(hi))
    if npix == 5 and nb == 64:
        assert float(b.min()) < 0 and float(b.max()) > 1 and int((b[0, 0, 0] == b[0, 0, 0].round()).sum()) > 8    # outside [0, 1], ties


def test_bounded_large_case_and_clip_before_sort_defect():
    """32 773 pixels (the size of the GPU test) pass the counted bar in float32 torch.  The clip moved in front of the sort alone changes nothing --
    clip is monotone, so sort(clip(v)) = clip(sort(v)) element for element, bit for bit (asserted): that is no defect of the function.  What is
    planted is the neighbouring slip that is one: the clip moved in front of the map as well, its bounds lo, hi applied to the unmapped b"""
    lo, hi = I.EXACT_RANGES[0]
    b = I.bounded_operands(32773, 64)
    ref, mag = I.bounded_bin_centers_ref(b, lo, hi)
    y = _run(lambda y: fake.bounded_bin_centers(b, y, lo, hi), tuple(b.shape))
    assert I.counted_bar(y, ref, mag, I.K_BOUNDED)[0]
    v = (hi - lo) * b + lo
    assert torch.equal(torch.sort(torch.clip(v, lo, hi), dim=-1)[0], y) and float(b.min()) < 0 and float(b.max()) > 1
    bad = torch.sort((hi - lo) * torch.clip(b, lo, hi) + lo, dim=-1)[0]
    assert not I.counted_bar(bad, ref, mag, I.K_BOUNDED)[0]
    old = float((bad - y).abs().max()) / 80.0 <= 1e-4
    print(f"bounded clip before sort: worst |d| / bound {I.counted_bar(bad, ref, mag, I.K_BOUNDED)[1]:.3g} | op_checks 1e-4 {'ACCEPTS' if old else 'rejects'}")


# ---- copies ----
def _truncate_bf16(x):
    return (x.view(torch.int32) & -65536).view(torch.float32).to(torch.bfloat16)


def test_bf16_copy_expectations_and_truncation_defect():
    """float32 -> bf16 is torch's round-to-nearest-even, bf16 -> float32 exact; the planted values separate it from truncation and from
    round-half-up; truncation passes op_checks.misc_ops' 1e-2 bar"""
    e = I.bf16_edge_values()
    want = torch.tensor([0x3F80, 0x3F82, 0xBF80, 0xBF82, 0x3F80, 0x3F81, 0x4000, 0x4000], dtype=torch.int32)
    got = e.to(torch.bfloat16).view(torch.int16).to(torch.int32) & 0xFFFF
    assert torch.equal(got, want)
    half_up = (((e.view(torch.int32).to(torch.int64) & 0xFFFFFFFF) + 0x8000) >> 16).to(torch.int32) & 0xFFFF
    assert not torch.equal(half_up, want)
    x = I.copy_operands((3, 5, 7, 24), torch.float32)
    y = x.to(torch.bfloat16)
    assert torch.equal(y.float().to(torch.bfloat16), y) and torch.equal(x[0, 0, 0, :8], e)
    bad = _truncate_bf16(x)
    assert not torch.equal(bad, y)
    assert I.counted_bar(y, x.double(), x.double().abs(), 0, bf16_out=True)[0] and not I.counted_bar(bad, x.double(), x.double().abs(), 0, bf16_out=True)[0]
    old = float((bad.float() - y.float()).abs().max()) / max(1.0, float(y.float().abs().max())) <= 1e-2
    print(f"bf16 copy by truncation: op_checks 1e-2 {'ACCEPTS' if old else 'rejects'}")
    assert old
    # add_rowwise: one float32 addition, then the rounding of the store
    xb, pos = I.copy_operands((3, 5, 24), torch.bfloat16), I.copy_operands((5, 24), torch.float32, seed=32)
    got = xb.clone()
    fake.add_rowwise(got, pos)
    assert torch.equal(got, (xb.float() + pos).to(torch.bfloat16))


# ---- mixed-dtype resize and RoI ----
MIXED_RESIZE_CASES = [I.RESIZE_CASES[0], I.RESIZE_CASES[1]]          # 14 x 19 -> 28 x 37 (up), 56 x 74 -> 28 x 37 (down)
MIXED_MODES = [(torch.float32, torch.bfloat16), (torch.bfloat16, torch.float32)]


@pytest.mark.parametrize("din,dout", MIXED_MODES, ids=["f32_to_bf16", "bf16_to_f32"])
@pytest.mark.parametrize("case", MIXED_RESIZE_CASES, ids=lambda c: "x".join(map(str, c)))
def test_float32_mixed_resize_passes_the_counted_bar(case, din, dout):
    h, w, oh, ow, C = case
    x, add = I.features((2, h, w, C), h, din), I.features((2, oh, ow, C), w + 1, dout)
    bf = dout == torch.bfloat16
    ref, mag = I.bilinear_ref(x, oh, ow)
    assert I.counted_bar(_run(lambda y: fake.resize(x, y), (2, oh, ow, C), dout), ref, mag, I.K_BILERP, bf)[0]
    ref, mag = I.bilinear_ref(x, oh, ow, add)
    assert I.counted_bar(_run(lambda y: fake.resize(x, y, add=add), (2, oh, ow, C), dout), ref, mag, I.K_BILERP_ADD, bf)[0]
