"""Evaluation side on the CPU (no GPU needed): the numpy restatements of tests/eval_side_ref.py pinned to the reference's own functions
(live under the `reference` marker, against tests/golden/eval_side.npz otherwise), the hand-written dilation KATs, and the host logic of
postprocess.get_boundaries / colorize_infer_pfv1 / colorize_rescale / DepthEvaluator driven through stand-in ops.

On the parent commit every test here fails at import or attribute lookup: tests/eval_side_ref.py, tests/golden/eval_side.npz,
postprocess.get_boundaries, colorize_infer_pfv1, colorize_rescale, DepthEvaluator and METRIC_KEYS do not exist there."""
import os

import numpy as np
import pytest
import torch

from patchfusion_amd import postprocess as post
from tests import eval_side_ref as R
from tests.fake_ops import ops as fake_base

G = np.load(os.path.join(os.path.dirname(__file__), "golden", "eval_side.npz"))
CMAPS = ("magma_r", "turbo_r", "gray_r")


class EvalFakeOps(type(fake_base)):
    """tests/fake_ops.py plus stand-ins for the two evalops.hip entry points"""

    @staticmethod
    def depth_boundaries(disp, th, dilation, out):
        if not 0 <= int(dilation) <= 32:
            raise ValueError("dilation")
        out[:] = torch.from_numpy(R.get_boundaries(disp.numpy(), th, int(dilation)))
        return out

    @staticmethod
    def colorize_ex(depth, vmin_vmax, lut_rgba, N, invalid_val, background_rgba, out, invalid_mask=None, layout=0):
        rgba = torch.empty(depth.shape + (4,), dtype=torch.uint8)
        fake_base.colorize(depth, vmin_vmax, lut_rgba, N, invalid_val, background_rgba, rgba, invalid_mask=invalid_mask)
        out[:] = rgba if layout == 0 else rgba[..., [2, 1, 0]]
        return out


fake = EvalFakeOps()


# ---------------------------------------------------------------- get_boundaries restatement
def _boundary_inputs():
    for (H, W) in R.BOUNDARY_SHAPES:
        for th in (1.0, 0.25):
            yield f"edges_{H}x{W}_th{th}", R.step_plane(H, W, th, seed=H * 1000 + W), th
        yield f"edges_special_{H}x{W}", R.special_plane(H, W, seed=H + W), 1.0


def test_boundary_restatement_matches_reference_fixture():
    n_edges = 0
    for key, d, th in _boundary_inputs():
        e = R.get_boundaries(d, th, 0)
        assert e.dtype == np.float32 and np.array_equal(e, G[key].astype(np.float32)), key
        n_edges += int(e.sum())
    assert n_edges > 1000                                            # the planes do have edges
    # the inputs carry what they promise: differences equal to th, one ulp above and one ulp below it
    d = R.step_plane(70, 130, 0.25, seed=70130)
    diffs = np.abs(np.diff(d, axis=1)).ravel()
    t = np.float32(0.25)
    assert (diffs == t).any() and (diffs == np.nextafter(t, np.float32(1))).any() and (diffs == np.nextafter(t, np.float32(0))).any()
    cols = np.nonzero(np.abs(np.diff(d, axis=1)).max(axis=0))[0] + 1
    assert {63, 64, 65, 128, 129} <= set(cols.tolist())              # tile seams of the kernel (64 columns) +-1
    rows = np.nonzero(np.abs(np.diff(d, axis=0)).max(axis=1))[0] + 1
    assert {31, 32, 33, 63, 64, 65} <= set(rows.tolist())


@pytest.mark.reference
def test_boundary_restatement_matches_reference_live():
    from oracle import ref_shim
    if not ref_shim.reference_available():
        pytest.skip("reference tree not present")
    ref_shim.import_reference()
    from estimator.utils.image_ops import get_boundaries           # cv2 is a stub here: dilation = 0 only, the dilated cases rest on the KATs
    for key, d, th in _boundary_inputs():
        with np.errstate(invalid="ignore"):
            ref = get_boundaries(d, th=th, dilation=0)
        mine = R.get_boundaries(d, th, 0)
        assert ref.dtype == mine.dtype and np.array_equal(ref, mine), key


def test_dilation_kats():
    """written out by hand from cv2.dilate's definition: anchor (k//2, k//2), window rows y-k//2 .. y-k//2+k-1"""
    e = np.zeros((40, 40), np.float32)
    e[20, 20] = 1
    want = np.zeros((40, 40), np.float32)
    want[16:26, 16:26] = 1                                           # k = 10: y-5 <= 20 <= y+4  <=>  16 <= y <= 25
    assert np.array_equal(R.dilate_box(e, 10), want)
    want = np.zeros((40, 40), np.float32)
    want[19:22, 19:22] = 1                                           # k = 3: symmetric
    assert np.array_equal(R.dilate_box(e, 3), want)
    want = np.zeros((40, 40), np.float32)
    want[20:22, 20:22] = 1                                           # k = 2: y-1 <= 20 <= y  <=>  y in {20, 21}
    assert np.array_equal(R.dilate_box(e, 2), want)
    assert np.array_equal(R.dilate_box(e, 1), e)
    # borders: a corner pixel with k = 10 spreads to rows / columns 0 .. 5 only (0-5 <= 0 <= y+4 and y >= 0)
    c = np.zeros((12, 9), np.float32)
    c[0, 0] = 1
    want = np.zeros((12, 9), np.float32)
    want[0:6, 0:6] = 1
    assert np.array_equal(R.dilate_box(c, 10), want)
    c = np.zeros((12, 9), np.float32)
    c[11, 8] = 1                                                     # y-5 <= 11 <= y+4: y in 7 .. 11 (16 cut by the image); x in 4 .. 8
    want = np.zeros((12, 9), np.float32)
    want[7:12, 4:9] = 1
    assert np.array_equal(R.dilate_box(c, 10), want)
    # through the threshold: one pixel of a 40x40 zero plane raised by 2 > th = 1 makes itself and its 4 neighbours edges (a plus
    # shape, rows / columns 19 .. 21), whose k = 10 dilation is the union of five 10x10 boxes: rows 15 .. 26 x columns 16 .. 25 and
    # rows 16 .. 25 x columns 15 .. 26
    d = np.zeros((40, 40), np.float32)
    d[20, 20] = 2
    assert np.array_equal(R.get_boundaries(d, 1., 10), plus_dilated_kat())


def plus_dilated_kat():
    want = np.zeros((40, 40), np.float32)
    want[15:27, 16:26] = 1
    want[16:26, 15:27] = 1
    return want


# ---------------------------------------------------------------- colour restatements and host logic
def test_colour_restatements_match_reference_fixture():
    d, clean, im = R.colour_plane(), R.colour_plane(invalid_frac=0.0), R.colour_mask()
    const = np.full((61, 83), 0.7031, np.float32)
    lo, hi = (np.float32(v) for v in G["pfv1_range"][:2])
    assert np.array_equal(R.colorize_infer_pfv1(clean, vmin=lo, vmax=hi), G["pfv1_fixed_range"])
    assert G["pfv1_fixed_range"].shape == (61, 83, 3)
    assert np.array_equal(R.colorize_infer_pfv1(const), G["pfv1_const"])
    for cmap in CMAPS:
        assert np.array_equal(R.colorize_rescale(d, cmap=cmap), G[f"rescale_{cmap}"]), cmap     # min / max are exact: no caveat
        for key, x, rng in ((f"pfv1_{cmap}", clean, G["pfv1_range"][:2]), (f"pfv1_inv_{cmap}", d, G["pfv1_range"][2:])):
            # the installed numpy's percentile, handed over as float32: exact
            assert np.array_equal(R.colorize_infer_pfv1(x, cmap=cmap, vmin=np.float32(rng[0]), vmax=np.float32(rng[1])), G[key]), key
            # own percentile (numpy 1.24 semantics): the bound colorize's tests use
            diff = np.abs(R.colorize_infer_pfv1(x, cmap=cmap).astype(int) - G[key].astype(int)).max(axis=-1)
            assert (diff > 0).mean() < 2e-3, key
    assert np.array_equal(R.colorize_rescale(const), G["rescale_const"])
    assert np.array_equal(R.colorize_rescale(d, gamma_corrected=True), G["rescale_gamma"])
    assert np.array_equal(R.colorize_rescale(d, invalid_mask=im), G["rescale_mask"])
    assert np.array_equal(R.colorize_rescale(d, cmap="magma_r", invalid_mask=im, gamma_corrected=True, value_transform=np.square,
                                             background_color=(10, 200, 30, 255)), G["rescale_all"])
    assert np.array_equal(G["rescale_tensor"], G["rescale_turbo_r"])
    # rescale's range includes the invalid -99: the valid pixels crowd the top of the map, unlike colorize's
    assert (G["rescale_turbo_r"][d == -99] == np.array([128, 128, 128, 255])).all()


def test_colour_host_logic_through_fake_ops():
    d, clean, im = torch.from_numpy(R.colour_plane()), torch.from_numpy(R.colour_plane(invalid_frac=0.0)), R.colour_mask()
    lo, hi = (float(np.float32(v)) for v in G["pfv1_range"][:2])
    img = post.colorize_infer_pfv1(clean, vmin=lo, vmax=hi, ops=fake)
    assert img.dtype == torch.uint8 and img.shape == (61, 83, 3) and np.array_equal(img.numpy(), G["pfv1_fixed_range"])
    assert np.array_equal(post.colorize_infer_pfv1(clean, cmap="gray_r", ops=fake).numpy(), R.colorize_infer_pfv1(clean.numpy(), cmap="gray_r"))
    for cmap in CMAPS:
        assert np.array_equal(post.colorize_rescale(d[None, None], cmap=cmap, ops=fake).numpy(), G[f"rescale_{cmap}"])
    assert np.array_equal(post.colorize_rescale(d, gamma_corrected=True, ops=fake).numpy(), G["rescale_gamma"])
    assert np.array_equal(post.colorize_rescale(d, invalid_mask=im, ops=fake).numpy(), G["rescale_mask"])
    assert np.array_equal(post.colorize_rescale(d, cmap="magma_r", invalid_mask=torch.from_numpy(im), gamma_corrected=True, value_transform=np.square,
                                                background_color=(10, 200, 30, 255), ops=fake).numpy(), G["rescale_all"])
    rgba = post.colorize(d, cmap="magma_r", ops=fake)
    assert torch.equal(post.colorize(d, cmap="magma_r", ops=fake, layout="bgr"), rgba[:, :, [2, 1, 0]])
    with pytest.raises(ValueError):
        post.colorize(d, ops=fake, layout="rgb")
    e = post.get_boundaries(torch.from_numpy(R.step_plane(37, 53, 1.0, 5))[None, None], 1, 3, ops=fake)
    assert e.dtype == torch.float32 and e.shape == (37, 53)
    with pytest.raises(ValueError):
        post.get_boundaries(torch.zeros(4, 4), 1, 33, ops=fake)


# ---------------------------------------------------------------- DepthEvaluator arithmetic
class SumsOps:
    """depth_metrics stand-in that writes prepared sums; records what the evaluator hands over"""

    def __init__(self, rows):
        self.rows, self.calls = list(rows), []

    def depth_metrics(self, gt, pred, edges, min_depth, max_depth, crop, out13, additional_mask=None):
        assert out13.dtype == torch.float64 and out13.numel() == 13
        self.calls.append(dict(edges=edges, crop=crop, lo=min_depth, hi=max_depth, mask=additional_mask))
        out13.copy_(torch.tensor(self.rows[len(self.calls) - 1], dtype=torch.float64))
        return out13

    def depth_boundaries(self, disp, th, dilation, out):
        return EvalFakeOps.depth_boundaries(disp, th, dilation, out)


def _sums(n, seed, n_edge=5.0):
    rs = np.random.RandomState(seed)
    s = [float(n)] + [float(v) for v in np.sort(rs.randint(0, n + 1, 3))] + [float(v) for v in rs.rand(7) * n]
    s[8] = -abs(s[8]) * 0.1                                          # S(err); S(err^2)/n - (S(err)/n)^2 stays positive
    s[9] = abs(s[9]) + 1.0
    return s + [float(rs.rand() * n_edge), float(n_edge)]


def test_depth_evaluator_results_and_summary_arithmetic():
    rows = [_sums(1000, 1), _sums(800, 2), [0.0] * 13, _sums(500, 3, n_edge=0.0), _sums(1200, 4)]     # image 2: n = 0, image 3: no edge pixel
    ops = SumsOps(rows)
    ev = post.DepthEvaluator(1e-3, 80, capacity=2, ops=ops)
    gt, pred, disp = (torch.from_numpy(a) for a in R.metric_case(0, 16, 24))
    edges = torch.zeros(16, 24)
    for i in range(5):
        assert ev.add(gt, pred, disp_gt_edges=edges) == i
    assert len(ev) == 5 and ev.capacity == 8 and all(c["crop"] == (0, 16, 0, 24) and c["edges"] is not None for c in ops.calls)
    res = ev.results()
    want = []
    for s in rows:
        r = post.metrics_from_sums(s)
        r["see"] = s[11] / s[12] if s[12] > 0 else 0.0
        want.append(r)
    assert [list(r) for r in res] == [list(post.METRIC_KEYS)] * 5
    for a, b in zip(res, want):
        for k in post.METRIC_KEYS:
            assert a[k] == b[k] or (np.isnan(a[k]) and np.isnan(b[k])), k
    assert all(np.isnan(res[2][k]) for k in post.METRIC_KEYS[:9]) and res[2]["see"] == 0.0 and res[3]["see"] == 0.0 and res[0]["see"] > 0
    summ = ev.summary()
    assert list(summ) == ["a1", "a2", "a3", "abs_rel", "rmse", "log_10", "rmse_log", "silog", "sq_rel", "see"]
    for j, k in enumerate(summ):
        ref = np.nanmean([list(r.values())[j] for r in want])        # pre_eval_to_metrics: positional columns of the dicts
        assert summ[k] == pytest.approx(ref, rel=1e-15, abs=0), k
    # disp_gt instead of edges: the boundary plane is made first; neither: no `see`
    ops2 = SumsOps([_sums(10, 5), _sums(10, 6)])
    ev2 = post.DepthEvaluator(1e-3, 80, garg_crop=True, ops=ops2)
    ev2.add(gt, pred, disp_gt=disp, th=0.5, dilation=3)
    ev2.add(gt, pred)
    assert torch.equal(ops2.calls[0]["edges"], torch.from_numpy(R.get_boundaries(disp.numpy(), 0.5, 3))) and ops2.calls[1]["edges"] is None
    assert ops2.calls[0]["crop"] == post.crop_rectangle(16, 24, True, False, "")
    r2 = ev2.results()
    assert "see" in r2[0] and "see" not in r2[1] and ev2.summary()["see"] == r2[0]["see"]
    assert post.DepthEvaluator(1e-3, 80, ops=ops2).results() == [] and "see" not in post.DepthEvaluator(1e-3, 80, ops=ops2).summary()


def test_depth_evaluator_matches_reference_metrics_fixture():
    """six images through tests/fake_ops.py's numpy depth_metrics: per-image dicts and the nanmean summary against the reference's own
    compute_metrics (rtol 2e-5 as tests/test_io_cpu.py: float32 terms summed in double here, pairwise in float32 by numpy)"""
    ev = post.DepthEvaluator(1e-3, 80, capacity=2, ops=fake)
    for i in range(6):
        gt, pred, disp = (torch.from_numpy(a) for a in R.metric_case(i))
        ev.add(gt[None, None], pred[None, None], disp_gt=disp, th=1, dilation=0)
    keys = [str(k) for k in G["metrics_keys"]]
    assert keys == list(post.METRIC_KEYS)
    res = ev.results()
    got = np.array([[r[k] for k in keys] for r in res])
    assert np.isnan(G["metrics"][2, :9]).all() and G["metrics"][2, 9] == 0 and G["metrics"][4, 9] == 0 and (G["metrics"][[0, 1, 3, 5], 9] > 0).all()
    np.testing.assert_allclose(got, G["metrics"], rtol=2e-5, equal_nan=True)
    summ = ev.summary()
    np.testing.assert_allclose([summ[k] for k in keys], np.nanmean(G["metrics"], axis=0), rtol=2e-5)
