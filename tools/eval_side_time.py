"""Times the evaluation-side kernels (csrc/evalops.hip) at 2160x3840 on one GPU and writes profiles/eval_side_time.json:

  * pf_depth_boundaries at dilation 0 and 10 and pf_depth_to_u16 (the pure streaming pass to compare with), device events over many
    launches, as time and as a share of their algorithmic bytes;
  * the host path the boundary kernel replaces: the numpy restatement of get_boundaries (tests/eval_side_ref.py; the reference's own
    function where the reference tree is present) plus the upload of the plane, wall clock;
  * a six-image metrics loop per image, compute_metrics (one device-to-host copy per image) against DepthEvaluator (one at the end),
    interleaved in one process.

    python tools/eval_side_time.py [--out profiles/eval_side_time.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def dev_time_us(fn, iters=50, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1000.0 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_side_time.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    from patchfusion_amd import postprocess as post
    from patchfusion_amd.hip_ops import ops
    from tests import eval_side_ref as R

    H, W = 2160, 3840
    rs = np.random.RandomState(0)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    gt = (5 + 3 * np.sin(xx / 160) * np.cos(yy / 120) + (xx > W // 2) * 4).astype(np.float32)
    disp = (200.0 / gt).astype(np.float32)
    d = torch.from_numpy(disp).cuda()
    out = torch.empty_like(d)
    u16 = torch.empty(d.shape, dtype=torch.uint16, device=d.device)
    px = H * W
    res = {"device": torch.cuda.get_device_name(0), "grid": [H, W], "note": "measured on one box"}
    for name, fn, nbytes in (("depth_boundaries_d0", lambda: ops.depth_boundaries(d, 1.0, 0, out), 8 * px),
                             ("depth_boundaries_d10", lambda: ops.depth_boundaries(d, 1.0, 10, out), 8 * px),
                             ("depth_boundaries_d32", lambda: ops.depth_boundaries(d, 1.0, 32, out), 8 * px),
                             ("depth_to_u16", lambda: ops.depth_to_u16(d, u16), 6 * px)):
        us = dev_time_us(fn)
        res[name] = {"us": round(us, 2), "algorithmic_bytes": nbytes, "TBps": round(nbytes / us / 1e6, 3)}
    lut, N = post.colormap_lut("magma_r", d.device)
    vmm = torch.tensor([float(disp.min()), float(disp.max())], device=d.device)
    bgr = torch.empty(px * 3, dtype=torch.uint8, device=d.device)
    us = dev_time_us(lambda: ops.colorize_ex(d, vmm, lut, N, -99, (128, 128, 128, 255), bgr, layout=ops.COLOR_BGR))
    res["colorize_bgr"] = {"us": round(us, 2), "algorithmic_bytes": 7 * px, "TBps": round(7 * px / us / 1e6, 3)}

    # the host path of the parent commit: numpy get_boundaries + upload
    host_fn, host_name = (lambda x: R.get_boundaries(x, 1.0, 0)), "tests/eval_side_ref.py restatement"
    try:
        from oracle import ref_shim
        if ref_shim.reference_available():
            ref_shim.import_reference()
            from estimator.utils.image_ops import get_boundaries as ref_gb
            host_fn, host_name = (lambda x: ref_gb(x, th=1.0, dilation=0)), "reference get_boundaries"
    except Exception:
        pass
    ts = []
    for _ in range(3):
        t0 = time.perf_counter()
        e = torch.from_numpy(host_fn(disp)).cuda()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    assert torch.equal(e, ops.depth_boundaries(d, 1.0, 0, out))
    res["host_get_boundaries_d0_plus_upload"] = {"function": host_name, "ms_min": round(min(ts) * 1e3, 2), "ms_all": [round(t * 1e3, 2) for t in ts]}

    # six-image metrics loop, interleaved A/B
    pred = torch.from_numpy((gt[::2, ::2] * (1 + 0.03 * rs.randn(H // 2, W // 2))).astype(np.float32)).cuda()
    g = torch.from_numpy(gt).cuda()
    kw = dict(min_depth_eval=1e-3, max_depth_eval=80, garg_crop=False, eigen_crop=False, dataset="")

    def loop_a():
        return [post.compute_metrics(g, pred, disp_gt_edges=post.get_boundaries(d, 1, 0), **kw) for _ in range(6)]

    def loop_b():
        ev = post.DepthEvaluator(1e-3, 80)
        for _ in range(6):
            ev.add(g, pred, disp_gt=d, th=1, dilation=0)
        return ev.results()

    ta, tb = [], []
    loop_a(), loop_b()
    for _ in range(10):
        for fn, acc in ((loop_a, ta), (loop_b, tb)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            acc.append((time.perf_counter() - t0) / 6)
    res["metrics_loop_per_image"] = {"what": "boundaries + metrics only (no tile pass), 10 interleaved repeats of 6 images",
                                     "compute_metrics_ms_median": round(float(np.median(ta)) * 1e3, 4),
                                     "depth_evaluator_ms_median": round(float(np.median(tb)) * 1e3, 4),
                                     "compute_metrics_ms_min_max": [round(min(ta) * 1e3, 4), round(max(ta) * 1e3, 4)],
                                     "depth_evaluator_ms_min_max": [round(min(tb) * 1e3, 4), round(max(tb) * 1e3, 4)]}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
