"""GPU checks of the evaluation side (csrc/evalops.hip, postprocess.get_boundaries / colorize_infer_pfv1 / colorize_rescale /
DepthEvaluator) against the numpy restatements of tests/eval_side_ref.py (pinned to the reference's own functions in
tests/test_eval_side_cpu.py) and the reference-made fixture tests/golden/eval_side.npz.  Everything here is comparisons, byte lookups
and order statistics, so every check is exact unless it says otherwise."""
import os

import numpy as np
import pytest
import torch

from tests import eval_side_ref as R

pytestmark = pytest.mark.gpu

G = np.load(os.path.join(os.path.dirname(__file__), "golden", "eval_side.npz"))
CMAPS = ("magma_r", "turbo_r", "gray_r")
DILATIONS = (0, 1, 2, 3, 10, 11, 32)
_REF = {}


def _mods():
    from patchfusion_amd import postprocess as post
    from patchfusion_amd.hip_ops import ops
    return post, ops


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _metric_inputs():
    """the six evaluator images on the device and the compute_metrics dict of each, computed once and left unchanged"""
    if "metrics" not in _REF:
        post, _ = _mods()
        imgs, dicts = [], []
        for i in range(6):
            gt, pred, disp = R.metric_case(i)
            edges = R.get_boundaries(disp, 1, 0)
            imgs.append(tuple(_cuda(a) for a in (gt, pred, disp, edges)))
            dicts.append(post.compute_metrics(imgs[-1][0], imgs[-1][1], min_depth_eval=1e-3, max_depth_eval=80, garg_crop=False, eigen_crop=False,
                                              dataset="", disp_gt_edges=imgs[-1][3]))
        _REF["metrics"] = (imgs, dicts)
    return _REF["metrics"]


def _same_dicts(a, b):
    assert list(a) == list(b), (list(a), list(b))
    for k in a:
        assert a[k] == b[k] or (np.isnan(a[k]) and np.isnan(b[k])), (k, a[k], b[k])


# ---------------------------------------------------------------- boundaries
@pytest.mark.parametrize("shape", R.BOUNDARY_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_boundaries_match_restatement(shape):
    post, _ = _mods()
    H, W = shape
    for th in (1.0, 0.25):
        d = R.step_plane(H, W, th, seed=H * 1000 + W)
        dev = _cuda(d)
        for k in DILATIONS:
            got = post.get_boundaries(dev, th, k)
            assert got.dtype == torch.float32 and got.shape == (H, W)
            assert np.array_equal(got.cpu().numpy(), R.get_boundaries(d, th, k)), (shape, th, k)
        assert np.array_equal(post.get_boundaries(dev, th, 0).cpu().numpy(), G[f"edges_{H}x{W}_th{th}"].astype(np.float32))   # the reference's own
    d = R.special_plane(H, W, seed=H + W)                             # NaN, +-inf
    for k in DILATIONS:
        assert np.array_equal(post.get_boundaries(_cuda(d), 1.0, k).cpu().numpy(), R.get_boundaries(d, 1.0, k)), (shape, "special", k)
    assert np.array_equal(post.get_boundaries(_cuda(d), 1.0, 0).cpu().numpy(), G[f"edges_special_{H}x{W}"].astype(np.float32))


def test_boundaries_kat_defaults_and_limits():
    """Hand-written KAT through the thresholding: pixel (20, 20) of a 40x40 zero plane raised by 2 > th = 1 makes itself and its four
    neighbours edges (rows / columns 19 .. 21, a plus); output y sees rows y-5 .. y+4, so an edge in row r reaches y = r-4 .. r+5: the
    k = 10 dilation is rows 15 .. 26 x columns 16 .. 25 united with rows 16 .. 25 x columns 15 .. 26.  With dilation 0 the plus itself."""
    post, ops = _mods()
    d = torch.zeros(40, 40)
    d[20, 20] = 2
    want = torch.zeros(40, 40)
    want[15:27, 16:26] = 1
    want[16:26, 15:27] = 1
    assert torch.equal(post.get_boundaries(d.cuda()).cpu(), want)     # defaults: th = 1, dilation = 10
    plus = torch.zeros(40, 40)
    plus[19:22, 20] = 1
    plus[20, 19:22] = 1
    assert torch.equal(post.get_boundaries(d.cuda(), 1., 0).cpu(), plus)
    d[20, 20] = 1                                                     # a jump of exactly th is no edge (strictly greater)
    assert float(post.get_boundaries(d.cuda(), 1., 10).sum()) == 0
    # [1,1,H,W] input and a non-contiguous view are squeezed / packed like the neighbouring functions do
    x = _cuda(R.step_plane(37, 53, 1.0, 3))
    assert torch.equal(post.get_boundaries(x[None, None], 1, 3), post.get_boundaries(x, 1, 3))
    assert torch.equal(post.get_boundaries(x.t(), 1, 3).cpu(), torch.from_numpy(R.get_boundaries(x.t().cpu().numpy(), 1, 3)))
    # beyond the LDS tile: an error, no fall-back -- in the wrapper and in the C entry point itself
    with pytest.raises(ValueError):
        post.get_boundaries(x, 1, 33)
    with pytest.raises(ValueError):
        post.get_boundaries(x, 1, -1)
    import ctypes as C
    import patchfusion_amd._lib as L
    out = torch.empty_like(x)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert L.load().pf_depth_boundaries(C.c_void_p(x.data_ptr()), 1, 37, 53, 1.0, 33, C.c_void_p(out.data_ptr()), st) == 1      # PF_ERR_ARG
    assert L.load().pf_depth_boundaries(C.c_void_p(x.data_ptr()), 1, 37, 53, 1.0, 32, C.c_void_p(out.data_ptr()), st) == 0
    with pytest.raises(L.PfError):
        ops.depth_boundaries(x.cpu(), 1, 0, torch.empty(37, 53))      # no CPU path


def test_device_boundaries_feed_the_metrics():
    """compute_metrics fed get_boundaries' device plane equals compute_metrics fed the host-made plane: the same kernel reads the same
    bytes (96x160 ground truth, pred at half resolution: the in-kernel resize runs too)"""
    post, _ = _mods()
    imgs, dicts = _metric_inputs()
    for i in (0, 3, 4):
        gt, pred, disp, edges = imgs[i]
        dev_edges = post.get_boundaries(disp, 1, 0)
        assert torch.equal(dev_edges, edges)
        r = post.compute_metrics(gt, pred, min_depth_eval=1e-3, max_depth_eval=80, garg_crop=False, eigen_crop=False, dataset="", disp_gt_edges=dev_edges)
        _same_dicts(r, dicts[i])
    assert dicts[0]["see"] > 0 and dicts[4]["see"] == 0.0


# ---------------------------------------------------------------- colour
def test_colorize_infer_pfv1_bit_exact():
    post, _ = _mods()
    d, clean = R.colour_plane(), R.colour_plane(invalid_frac=0.0)
    const = np.full((61, 83), 0.7031, np.float32)
    lo, hi = (float(np.float32(v)) for v in G["pfv1_range"][:2])
    img = post.colorize_infer_pfv1(_cuda(clean), vmin=lo, vmax=hi)
    assert img.dtype == torch.uint8 and img.shape == (61, 83, 3) and np.array_equal(img.cpu().numpy(), G["pfv1_fixed_range"])
    assert np.array_equal(post.colorize_infer_pfv1(_cuda(const)).cpu().numpy(), G["pfv1_const"])            # vmin == vmax: all 0
    for cmap in CMAPS:
        for key, x, rng in ((f"pfv1_{cmap}", clean, G["pfv1_range"][:2]), (f"pfv1_inv_{cmap}", d, G["pfv1_range"][2:])):
            got = post.colorize_infer_pfv1(_cuda(x), cmap=cmap).cpu().numpy()                                 # own minimum and 95th percentile
            assert np.array_equal(got, R.colorize_infer_pfv1(x, cmap=cmap)), key
            # the reference image was made with the installed numpy's percentile (DESIGN 9b caveat): exact with its range handed over,
            # colorize's bound (tests/test_io_cpu.py, tests/test_oracle_io.py) with the kernel's own
            fixed = post.colorize_infer_pfv1(_cuda(x), cmap=cmap, vmin=float(np.float32(rng[0])), vmax=float(np.float32(rng[1])))
            assert np.array_equal(fixed.cpu().numpy(), G[key]), key
            assert (np.abs(got.astype(int) - G[key].astype(int)).max(axis=-1) > 0).mean() < 2e-3, key


def test_colorize_rescale_bit_exact():
    post, _ = _mods()
    d, im = R.colour_plane(), R.colour_mask()
    const = np.full((61, 83), 0.7031, np.float32)
    dev = _cuda(d)
    for cmap in CMAPS:
        img = post.colorize_rescale(dev, cmap=cmap)
        assert img.dtype == torch.uint8 and img.shape == (61, 83, 4) and np.array_equal(img.cpu().numpy(), G[f"rescale_{cmap}"]), cmap
    assert np.array_equal(post.colorize_rescale(dev[None, None]).cpu().numpy(), G["rescale_tensor"])
    assert np.array_equal(post.colorize_rescale(_cuda(const)).cpu().numpy(), G["rescale_const"])
    assert np.array_equal(post.colorize_rescale(dev, gamma_corrected=True).cpu().numpy(), G["rescale_gamma"])
    assert np.array_equal(post.colorize_rescale(dev, invalid_mask=im).cpu().numpy(), G["rescale_mask"])
    assert np.array_equal(post.colorize_rescale(dev, cmap="magma_r", invalid_mask=_cuda(im), gamma_corrected=True, value_transform=np.square,
                                                background_color=(10, 200, 30, 255)).cpu().numpy(), G["rescale_all"])
    assert np.array_equal(post.colorize_rescale(dev, vmin=1.0, vmax=5.0, cmap="gray_r").cpu().numpy(), R.colorize_rescale(d, vmin=1.0, vmax=5.0, cmap="gray_r"))


def test_bgr_layout_and_unchanged_rgba_entry_point():
    from oracle import io_oracle
    post, ops = _mods()
    d, im = R.colour_plane(), R.colour_mask()
    dev = _cuda(d)
    for kw in (dict(cmap="magma_r"), dict(cmap="gray_r", invalid_mask=im), dict(cmap="turbo_r", gamma_corrected=True, background_color=(10, 200, 30, 255))):
        rgba = post.colorize(dev, **kw)
        assert np.array_equal(rgba.cpu().numpy(), io_oracle.colorize(d, **kw))                                # pf_colorize_f32: as before
        bgr = post.colorize(dev, layout="bgr", **kw)
        assert bgr.shape == (61, 83, 3) and torch.equal(bgr, rgba[:, :, [2, 1, 0]])
    # every tail length of the 4-pixel groups, and the RGBA layout of the extended entry point = the old entry point's bytes
    lut, N = post.colormap_lut("magma_r", dev.device)
    vmm = torch.tensor([1.0, 5.0], device=dev.device)
    for n in (1, 2, 3, 4, 5, 6, 7, 1021, 5063):
        x = dev.reshape(-1)[:n].contiguous()
        old = ops.colorize(x, vmm, lut, N, -99, (128, 128, 128, 255), torch.empty(n, 4, dtype=torch.uint8, device=dev.device))
        guard = torch.full((n * 3 + 16,), 77, dtype=torch.uint8, device=dev.device)
        ops.colorize_ex(x, vmm, lut, N, -99, (128, 128, 128, 255), guard[:n * 3], layout=ops.COLOR_BGR)
        assert torch.equal(guard[:n * 3].view(n, 3), old[:, [2, 1, 0]]) and bool((guard[n * 3:] == 77).all()), n
        new = ops.colorize_ex(x, vmm, lut, N, -99, (128, 128, 128, 255), torch.empty(n, 4, dtype=torch.uint8, device=dev.device), layout=ops.COLOR_RGBA)
        assert torch.equal(new, old), n


def test_percentile_0_and_100_are_the_extrema():
    """the ranges of colorize_infer_pfv1 / colorize_rescale rest on this: the radix select returns order statistics"""
    _, ops = _mods()
    rs = np.random.RandomState(7)
    x = (rs.randn(100003) * 5).astype(np.float32)
    x[rs.randint(0, x.size, 5000)] = x[rs.randint(0, x.size, 5000)]                                         # duplicates
    x[:50], x[50:100] = 0.0, -0.0
    x[100:110] = np.float32(1e-40) * np.arange(1, 11, dtype=np.float32)                                     # subnormals
    x[110:120] = -x[100:110]
    x[200:203] = x.max()
    x[300:303] = x.min()                                                                                    # the extrema occur more than once
    for v in (x, np.abs(x), -np.abs(x), x[100:120].copy(), np.concatenate([x[:100], x[100:110]])):
        got = ops.percentiles(_cuda(v), 0, 100).cpu().numpy()
        assert got[0] == v.min() and got[1] == v.max(), (got, v.min(), v.max())
        assert got.view(np.int32)[0] == v.min().view(np.int32) or v.min() == 0                              # +-0 compare equal; either is the minimum


# ---------------------------------------------------------------- evaluator
def test_depth_evaluator_six_images_growth_and_no_sync():
    post, _ = _mods()
    imgs, dicts = _metric_inputs()
    ev = post.DepthEvaluator(1e-3, 80, garg_crop=False, eigen_crop=False, dataset="", capacity=2)
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for i, (gt, pred, disp, edges) in enumerate(imgs):
            if i % 2:
                ev.add(gt, pred, disp_gt_edges=edges)                 # ready-made edges
            else:
                ev.add(gt[None, None], pred[None, None], disp_gt=disp, th=1., dilation=0)       # made on the device inside add
        with pytest.raises(RuntimeError):
            ev.results()                                              # the one copy to the host is here, not in add
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert len(ev) == 6 and ev.capacity == 8                          # grew 2 -> 4 -> 8
    res = ev.results()
    assert len(res) == 6
    for a, b in zip(res, dicts):
        _same_dicts(a, b)
    assert all(np.isnan(res[2][k]) for k in post.METRIC_KEYS[:9]) and res[2]["see"] == 0.0 and res[4]["see"] == 0.0 and res[0]["see"] > 0
    summ = ev.summary()
    assert list(summ) == list(post.METRIC_KEYS)
    for k in summ:
        np.testing.assert_allclose(summ[k], np.nanmean([r[k] for r in dicts]), rtol=1e-12, atol=0)
    # and against the reference's own compute_metrics (rtol 2e-5 as tests/test_io_gpu.py: float32 terms summed in double here)
    np.testing.assert_allclose(np.array([[r[k] for k in post.METRIC_KEYS] for r in res]), G["metrics"], rtol=2e-5, equal_nan=True)
    assert "libpf_hip.so" in open("/proc/self/maps").read()
