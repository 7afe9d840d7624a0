"""TEST INFRASTRUCTURE ONLY.  Generates tests/golden/eval_side.npz by running the REFERENCE'S OWN PYTHON for the evaluation side
(csrc/evalops.hip, postprocess.get_boundaries / colorize_infer_pfv1 / colorize_rescale / DepthEvaluator) on the seeded inputs of
tests/eval_side_ref.py:

  get_boundaries()       estimator/utils/image_ops.py:25-36   (dilation=0 only: cv2 is a stub in the build container)
  colorize_infer_pfv1()  estimator/utils/color.py:8-25
  colorize_rescale()     estimator/utils/color.py:28-93
  compute_metrics()      estimator/utils/metric.py:87-148     (six images, edges from the reference's get_boundaries)

Run in the build container only:   python tools/make_golden_eval.py
NOTE: executes under the installed numpy / matplotlib, not the versions the reference pins; np.percentile inside
colorize_infer_pfv1 is the installed numpy's.  The fixture records it (pfv1_range) so tests can separate the two effects, exactly as
oracle/make_golden_io.py does for colorize.  Only inputs that cannot be regenerated from a seed are stored; the inputs themselves come
from tests/eval_side_ref.py on both sides.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_shim  # noqa: E402
from tests import eval_side_ref as R  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "eval_side.npz")
CMAPS = ("magma_r", "turbo_r", "gray_r")


def reference_functions():
    ref_shim.import_reference()
    import matplotlib
    import matplotlib.cm
    if not hasattr(matplotlib.cm, "get_cmap"):                       # removed in matplotlib 3.9; the reference pins 3.7
        matplotlib.cm.get_cmap = lambda name: matplotlib.colormaps[name]
    from estimator.utils.color import colorize_infer_pfv1, colorize_rescale
    from estimator.utils.image_ops import get_boundaries
    from estimator.utils.metric import compute_metrics
    return get_boundaries, colorize_infer_pfv1, colorize_rescale, compute_metrics


def main():
    get_boundaries, colorize_infer_pfv1, colorize_rescale, compute_metrics = reference_functions()
    out = {}
    # ---- boundaries, dilation 0 ----
    for (H, W) in R.BOUNDARY_SHAPES:
        for th in (1.0, 0.25):
            out[f"edges_{H}x{W}_th{th}"] = get_boundaries(R.step_plane(H, W, th, seed=H * 1000 + W), th=th, dilation=0).astype(np.uint8)
        with np.errstate(invalid="ignore"):
            out[f"edges_special_{H}x{W}"] = get_boundaries(R.special_plane(H, W, seed=H + W), th=1.0, dilation=0).astype(np.uint8)

    # ---- colour ----
    d = R.colour_plane()
    clean = R.colour_plane(invalid_frac=0.0)
    const = np.full((61, 83), 0.7031, np.float32)
    im = R.colour_mask()
    out["pfv1_range"] = np.array([clean.min(), np.percentile(clean, 95), d.min(), np.percentile(d, 95)], dtype=np.float64)
    for cmap in CMAPS:
        out[f"pfv1_{cmap}"] = np.ascontiguousarray(colorize_infer_pfv1(clean.copy(), cmap=cmap))
        out[f"pfv1_inv_{cmap}"] = np.ascontiguousarray(colorize_infer_pfv1(d.copy(), cmap=cmap))          # -99 is an ordinary value here
        out[f"rescale_{cmap}"] = colorize_rescale(d.copy(), cmap=cmap)
    # the same with the range given as float32 values: independent of the installed numpy's percentile
    lo, hi = (float(np.float32(v)) for v in out["pfv1_range"][:2])
    out["pfv1_fixed_range"] = np.ascontiguousarray(colorize_infer_pfv1(clean.copy(), vmin=lo, vmax=hi))
    out["pfv1_const"] = np.ascontiguousarray(colorize_infer_pfv1(const.copy()))
    out["rescale_const"] = colorize_rescale(const.copy())
    out["rescale_gamma"] = colorize_rescale(d.copy(), gamma_corrected=True)
    out["rescale_mask"] = colorize_rescale(d.copy(), invalid_mask=im.copy())
    out["rescale_all"] = colorize_rescale(d.copy(), cmap="magma_r", invalid_mask=im.copy(), gamma_corrected=True, value_transform=np.square,
                                          background_color=(10, 200, 30, 255))
    out["rescale_tensor"] = colorize_rescale(torch.from_numpy(d)[None, None])

    # ---- six images through compute_metrics (u4k_dataset.py:185-186 arguments) ----
    keys = None
    rows = []
    for i in range(6):
        gt, pred, disp = R.metric_case(i)
        edges = get_boundaries(disp, th=1, dilation=0)
        with np.errstate(all="ignore"):
            r = compute_metrics(torch.from_numpy(gt)[None, None], torch.from_numpy(pred.copy())[None, None], disp_gt_edges=torch.from_numpy(edges)[None],
                                min_depth_eval=1e-3, max_depth_eval=80, garg_crop=False, eigen_crop=False, dataset="")
        keys = list(r.keys())
        rows.append([float(r[k]) for k in keys])
    out["metrics_keys"] = np.array(keys)
    out["metrics"] = np.array(rows, dtype=np.float64)
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes;", len(out), "arrays")


if __name__ == "__main__":
    main()
