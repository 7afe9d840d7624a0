"""Numpy restatements of the evaluation-side reference functions, for tests/test_eval_side_{cpu,gpu}.py (TEST INFRASTRUCTURE ONLY).

  get_boundaries       estimator/utils/image_ops.py:25-36 (= utils/metric.py:74-85)
  colorize_infer_pfv1  estimator/utils/color.py:8-25
  colorize_rescale     estimator/utils/color.py:28-93

Pinning: tests/test_eval_side_cpu.py compares each of them bit for bit with the reference's own function -- live where the reference
tree is present, against tests/golden/eval_side.npz (made by tools/make_golden_eval.py from the reference's own functions) otherwise.
cv2 is not installed where this was written, so the dilation follows cv2.dilate's documented definition (anchor (k//2, k//2), pixels
outside the image never raise a maximum): parity unpinned against OpenCV itself, pinned by the hand-written KATs of the two test
modules.  The colour functions reuse oracle/io_oracle.py (matplotlib's byte lookup, numpy 1.24's percentile), pinned in
tests/test_oracle_io.py."""
import numpy as np

from oracle import io_oracle


def threshold_edges(disp, th):
    """1.0 where |v - neighbour| > th for an up / down / left / right neighbour inside the image (float32 differences)"""
    d = np.asarray(disp, dtype=np.float32)
    H, W = d.shape
    e = np.zeros((H, W), bool)
    with np.errstate(invalid="ignore"):
        if H > 1:
            v = np.abs(d[1:, :] - d[:-1, :]) > np.float32(th)
            e[1:, :] |= v
            e[:-1, :] |= v
        if W > 1:
            h = np.abs(d[:, 1:] - d[:, :-1]) > np.float32(th)
            e[:, 1:] |= h
            e[:, :-1] |= h
    return e.astype(np.float32)


def dilate_box(edges, k):
    """cv2.dilate(edges, np.ones((k, k), np.uint8), iterations=1) by its definition: out[y, x] = max of edges over rows
    y - k//2 .. y - k//2 + k - 1 and columns x - k//2 .. x - k//2 + k - 1, outside pixels ignored (edges >= 0: pad with 0)"""
    H, W = edges.shape
    a = k // 2
    pad = np.zeros((H + k - 1, W + k - 1), edges.dtype)
    pad[a:a + H, a:a + W] = edges
    out = np.zeros_like(edges)
    for j in range(k):
        for i in range(k):
            np.maximum(out, pad[j:j + H, i:i + W], out=out)
    return out


def get_boundaries(disp, th=1., dilation=10):
    e = threshold_edges(disp, th)
    return dilate_box(e, dilation) if dilation > 0 else e


def _lookup(x, cmap):
    lut, N = io_oracle.colormap_lut_bytes(cmap)
    return io_oracle.colormap_bytes(x, lut, N)


def colorize_infer_pfv1(value, cmap="magma_r", vmin=None, vmax=None):
    """color.py:8-25 -> (H, W, 3) uint8, B G R.  vmax: numpy 1.24's percentile as in oracle/io_oracle.py (DESIGN 9b caveat)."""
    v = np.asarray(value, dtype=np.float32)
    vmin = v.min() if vmin is None else np.float32(vmin)
    vmax = io_oracle.percentile_linear(v, 95) if vmax is None else np.float32(vmax)
    x = (v - vmin) / (vmax - vmin) if vmin != vmax else v * np.float32(0.)
    return _lookup(x, cmap)[:, :, :3][..., ::-1]


def colorize_rescale(value, vmin=None, vmax=None, cmap="turbo_r", invalid_val=-99, invalid_mask=None, background_color=(128, 128, 128, 255),
                     gamma_corrected=False, value_transform=None, vminp=2, vmaxp=95):
    """color.py:28-93 -> (H, W, 4) uint8: colorize with vmin / vmax = min / max over all values, invalid ones included"""
    v = np.asarray(value, dtype=np.float32).squeeze()
    return io_oracle.colorize(v, vmin=v.min() if vmin is None else vmin, vmax=v.max() if vmax is None else vmax, cmap=cmap,
                              invalid_val=invalid_val, invalid_mask=invalid_mask, background_color=background_color,
                              gamma_corrected=gamma_corrected, value_transform=value_transform)


# ---------------------------------------------------------------- seeded inputs shared by the CPU and the GPU module
BOUNDARY_SHAPES = ((37, 53), (1, 64), (64, 1), (7, 5), (70, 130), (129, 257))
TILE_H, TILE_W = 32, 64            # the kernel's block tile (csrc/evalops.hip BD_TH x BD_TW): jumps are put on its seams


def step_plane(H, W, th, seed):
    """piecewise-constant float32 plane: a sum of row steps and column steps whose heights are exactly th, the next float32 above th
    and the next below (and their negatives), at random positions plus the image border and every multiple of the tile size +-1"""
    rs = np.random.RandomState(seed)
    t = np.float32(th)
    heights = np.array([t, np.nextafter(t, np.float32(np.inf)), np.nextafter(t, np.float32(0)), 2 * t, t / 2], np.float32)
    heights = np.concatenate([heights, -heights])

    def cuts(n, tile):
        c = set(rs.randint(1, n, size=max(1, n // 9)).tolist()) if n > 1 else set()
        c |= {1, n - 1}
        for m in range(tile, n + 2, tile):
            c |= {m - 1, m, m + 1}
        return sorted(x for x in c if 1 <= x < n)

    # running sums from 0: the first steps are the heights themselves, later ones are the heights up to one rounding of the sum, so
    # differences equal to th, one ulp above and one ulp below all occur
    row = np.zeros(H, np.float32)
    for y in cuts(H, TILE_H):
        row[y:] = row[y:] + heights[rs.randint(len(heights))]
    col = np.zeros(W, np.float32)
    for x in cuts(W, TILE_W):
        col[x:] = col[x:] + heights[rs.randint(len(heights))]
    d = np.zeros((H, W), np.float32)
    # steps that hold on a random band only, so that rows and columns differ
    y0, y1 = sorted(rs.randint(0, H + 1, 2))
    x0, x1 = sorted(rs.randint(0, W + 1, 2))
    d[:, :] = col[None, :]
    d[y0:y1, :] = (col * np.float32(0.5))[None, :]
    d[:, x0:x1] += row[:, None]
    # isolated pixels
    for _ in range(max(1, H * W // 200)):
        d[rs.randint(H), rs.randint(W)] += heights[rs.randint(len(heights))]
    return d


def special_plane(H, W, seed):
    """step plane with a few NaN and +-inf values (next to each other too: inf - inf = NaN is no edge)"""
    d = step_plane(H, W, 1.0, seed)
    rs = np.random.RandomState(seed + 1000)
    for v in (np.nan, np.inf, -np.inf, np.inf, np.nan):
        d[rs.randint(H), rs.randint(W)] = v
    if W >= 4:
        d[H // 2, 1:4] = (np.inf, np.inf, -np.inf)
    d[0, 0] = np.nan
    d[H - 1, W - 1] = np.inf
    return d


def colour_plane(H=61, W=83, seed=11, invalid_frac=0.03):
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    d = (3.0 + 2.0 * np.sin(xx / 9.0) * np.cos(yy / 7.0) + 0.01 * xx + rs.rand(H, W) * 0.5).astype(np.float32)
    if invalid_frac:
        d[rs.rand(H, W) < invalid_frac] = -99
    return d


def colour_mask(H=61, W=83, seed=12):
    m = np.random.RandomState(seed).rand(H, W) < 0.05
    m[10:20, 30:50] = True
    return m


def metric_case(i, H=96, W=160):
    """image i of the evaluator tests: (gt, pred at half resolution, disp) float32; image 2 has no valid ground truth, image 4 a
    constant disparity (no edges).

    The values are chosen so that every sum of pf_depth_metrics is EXACT in float64, whatever the order in which the kernel's blocks
    add their partial sums (atomics): gt lies in [3, 8], pred in [8.4, 32] (bilinear resizing stays inside the hull), so each of the
    eleven float32 terms stays within a band of at most 12 binary exponents (e.g. (ln gt - ln pred)^2 in [0.0023, 5.7], |gt - pred|
    in [0.4, 29]); a float32 term has 24 significant bits and at most 2^14 pixels are summed, so every partial sum fits in
    24 + 12 + 14 = 50 < 53 bits.  Only then can two runs of the same kernel be compared bit for bit."""
    rs = np.random.RandomState(100 + i)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    gt = (4.0 + np.sin(xx / (13.0 + i)) * np.cos(yy / 9.0) + (xx > W // 2 + 3 * i) * 3.0).astype(np.float32)
    gt[:3] = 0.0
    if i == 2:
        gt[:] = 0.0
    ph, pw = H // 2, W // 2
    pred = np.clip(8.4 + 23.6 * rs.rand(ph, pw), 8.4, 32.0).astype(np.float32)
    disp = np.full((H, W), 2.5, np.float32) if i == 4 else (40.0 / np.maximum(gt, 1.0)).astype(np.float32)
    return gt, pred, disp
