"""pytest -m gpu: the kernels that write the input of an fp16x2 Winograd layer also emit its channel maxima (csrc/imageops.hip: resize_src_kernel,
roi_align_kernel, copy_channels_kernel through the pf_*_ex entry points).

Per kernel: the vector the kernel merges equals pf_wino_absmax (the range pass) of the finished destination slice BIT FOR BIT, the destination has the
bits of the plain call, and a second run into the re-zeroed vector gives the same vector (no stale state).  Shapes: odd sizes that are no multiple of
any block shape, an ROI partly outside the map, a channel slice at a non-zero offset of a wider buffer, a channel that is all zero and one that is all
negative.  Every comparison is torch.equal."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _absmax(t):
    """the range pass over the NHWC float32 view t (any pixel stride): uint32 float bits per channel, as int32"""
    from patchfusion_amd import _lib, hip_ops
    L = _lib.load()
    Cc = t.shape[-1]
    cm = torch.zeros(Cc, dtype=torch.int32, device=DEV)
    npix = t.numel() // Cc
    hip_ops.check(L.pf_wino_absmax(C.c_void_p(t.data_ptr()), t.stride(-2), npix, Cc, 0, C.c_void_p(cm.data_ptr()), None), "pf_wino_absmax")
    torch.cuda.synchronize()
    return cm


def _check(run, dst_slice, plain):
    """run(cmax) writes the destination and merges into cmax; plain = the destination as the call without cmax wrote it"""
    Cc = dst_slice.shape[-1]
    cm = torch.full((Cc + 8,), 0x12345678, dtype=torch.int32, device=DEV)      # (+ 8 guard words the kernel must not touch)
    vecs = []
    for _ in range(2):
        cm[:Cc].zero_()
        dst_slice.fill_(float("nan"))
        run(cm[:Cc])
        torch.cuda.synchronize()
        assert torch.equal(dst_slice, plain), "the maxima-merging kernel changed the values it stores"
        assert torch.equal(cm[Cc:], torch.full((8,), 0x12345678, dtype=torch.int32, device=DEV)), "wrote past the vector"
        ref = _absmax(dst_slice)
        assert torch.equal(cm[:Cc], ref), (cm[:Cc] - ref).nonzero().flatten().tolist()[:8]
        # (the range pass itself, against torch: max |x| per channel)
        assert torch.equal(ref.view(torch.float32), dst_slice.abs().amax(dim=tuple(range(dst_slice.dim() - 1))))
        vecs.append(cm[:Cc].clone())
    assert torch.equal(vecs[0], vecs[1])
    return vecs[0]


def _special(x, kind):
    """a whole channel of zeros / a channel that is negative everywhere"""
    if kind == "zero":
        x[..., 3] = 0.0
    elif kind == "negative":
        x[..., 5] = -x[..., 5].abs() - 0.25
    return x


KINDS = ["plain", "zero", "negative"]


@pytest.mark.parametrize("kind", KINDS)
def test_resize_concat_emits_the_range_pass(kind):
    from patchfusion_amd.hip_ops import ops
    g = torch.Generator().manual_seed(1)
    B, H, W, OH, OW = 2, 13, 19, 27, 37
    xs = [torch.randn(B, H, W, c, generator=g) * s for c, s in ((32, 1.0), (64, 1e-3), (64, 300.0))]
    xs = [x.to(DEV) for x in xs]
    xs[0] = _special(xs[0], kind)
    xs[2] = _special(xs[2], kind)
    # a third source of another size, as the decoder's encoder map is
    xs[1] = (torch.randn(B, 7, 10, 64, generator=g) * 1e-3).to(DEV)
    y = torch.full((B, OH, OW, 160), float("nan"), device=DEV)
    ops.resize_concat(xs, y)
    torch.cuda.synchronize()
    plain = y.clone()
    assert not torch.isnan(plain).any()
    cm = _check(lambda c: ops.resize_concat(xs, y, cmax=c), y, plain)
    if kind == "zero":
        assert int(cm[3]) == 0 and int(cm[96 + 3]) == 0
    if kind == "negative":
        assert float(cm.view(torch.float32)[5]) >= 0.25


@pytest.mark.parametrize("kind", KINDS)
def test_resize_into_a_channel_slice_emits_the_range_pass(kind):
    """pf_resize_bilinear_ex, with and without the fused add, into channels [8, 72) of a wider buffer"""
    from patchfusion_amd.hip_ops import ops
    g = torch.Generator().manual_seed(2)
    B, H, W, OH, OW, Cc = 2, 13, 19, 27, 37, 64
    x = _special(torch.randn(B, H, W, Cc, generator=g).to(DEV), kind)
    add = torch.randn(B, OH, OW, Cc, generator=g).to(DEV)
    if kind == "zero":
        add[..., 3] = 0.0
    buf = torch.full((B, OH, OW, 96), float("nan"), device=DEV)
    y = buf[..., 8:72]
    for a in (None, add):
        ops.resize(x, y, add=a)
        torch.cuda.synchronize()
        plain = y.clone()
        cm = _check(lambda c: ops.resize(x, y, add=a, cmax=c), y, plain)
        if kind == "zero":
            assert int(cm[3]) == 0
    assert torch.isnan(buf[..., :8]).all() and torch.isnan(buf[..., 72:]).all()


@pytest.mark.parametrize("kind", KINDS)
def test_roi_align_emits_the_range_pass(kind):
    from patchfusion_amd.hip_ops import ops
    g = torch.Generator().manual_seed(3)
    H, W, Cc, oh, ow = 24, 40, 64, 27, 37
    feat = _special((torch.randn(1, H, W, Cc, generator=g) * 10).to(DEV), kind)
    # (batch index, x0, y0, x1, y1): one ROI inside the map (up-sampled), one that sticks out of it on two sides
    rois = torch.tensor([[0, 4.0, 3.0, 14.0, 9.0], [0, 30.0, 15.0, 52.0, 31.0]], dtype=torch.float32, device=DEV)
    buf = torch.full((2, oh, ow, 2 * Cc), float("nan"), device=DEV)
    y = buf[..., Cc:]
    ops.roi_align(feat, rois, y, 1.0)
    torch.cuda.synchronize()
    plain = y.clone()
    assert not torch.isnan(plain).any() and bool((plain[1, -1] == 0).all()), "the second ROI's last row lies outside the map"
    cm = _check(lambda c: ops.roi_align(feat, rois, y, 1.0, cmax=c), y, plain)
    if kind == "zero":
        assert int(cm[3]) == 0
    assert torch.isnan(buf[..., :Cc]).all()


@pytest.mark.parametrize("kind", KINDS)
def test_copy_channels_emits_the_range_pass(kind):
    from patchfusion_amd.hip_ops import ops
    g = torch.Generator().manual_seed(4)
    B, H, W, Cc = 1, 5, 103, 72                                     # 515 pixels: no multiple of 256; 9 channel vectors: the thread's vector changes
    x = _special((torch.randn(B, H, W, Cc, generator=g) * 1e4).to(DEV), kind)
    buf = torch.full((B, H, W, 136), float("nan"), device=DEV)
    y = buf[..., 40:112]
    ops.copy_channels(x, y)
    torch.cuda.synchronize()
    plain = y.clone()
    assert torch.equal(plain, x)
    cm = _check(lambda c: ops.copy_channels(x, y, cmax=c), y, plain)
    if kind == "zero":
        assert int(cm[3]) == 0
    assert torch.isnan(buf[..., :40]).all() and torch.isnan(buf[..., 112:]).all()


def test_producers_of_one_concat_buffer_fill_one_vector():
    """cat = [roi_align | copy_channels], as the fusion convs read it: two producers, each given its slice of ONE vector = the range pass over cat"""
    from patchfusion_amd.hip_ops import ops
    g = torch.Generator().manual_seed(5)
    H, W, Cc, oh, ow = 12, 20, 64, 24, 40
    feat = torch.randn(1, H, W, Cc, generator=g).to(DEV)
    fine = (torch.randn(2, oh, ow, Cc, generator=g) * 50).to(DEV)
    rois = torch.tensor([[0, 0.0, 0.0, 10.0, 6.0], [0, 10.0, 6.0, 20.0, 12.0]], dtype=torch.float32, device=DEV)
    cat = torch.full((2, oh, ow, 2 * Cc), float("nan"), device=DEV)
    cm = torch.zeros(2 * Cc, dtype=torch.int32, device=DEV)
    ops.roi_align(feat, rois, cat[..., :Cc], 1.0, cmax=cm[:Cc])
    ops.copy_channels(fine, cat[..., Cc:], cmax=cm[Cc:])
    torch.cuda.synchronize()
    assert torch.equal(cm, _absmax(cat))
