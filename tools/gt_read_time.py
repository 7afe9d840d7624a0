"""Times groundtruth.read_depth_gt (with edges) for one dataset at its native size, from the file's bytes in memory, against the host
path it replaces, and appends one JSON line to profiles/gt_read_time.jsonl:

  u4k 2160x3840 float32 .npy | eth3d 4032x6048 raw float32 | mid 1988x2964 PFM | gta 1080x1920 16-bit PNG | cityscapes 1024x2048 16-bit PNG

  * device reader: read_depth_gt(bytes, ...), wall clock with a device synchronisation before and after;
  * comparator: the numpy restatement of the reference's loader (tests/gt_ref.py) followed by the upload of depth and edges, the same way;
    the two run INTERLEAVED in one process, one warm-up each, then the median of --runs (>= 9) runs;
  * of the new path, separately: the upload of the payload alone (wall clock), and the conversion and boundary kernels on resident
    tensors (device events over many launches); the conversion kernel's achieved GB/s over its algorithmic bytes (payload read + planes
    written) next to the 8 TB/s of the specification.
The device planes are compared with the comparator's bit for bit before anything is timed.

The PNG files are written with filter type 0 on every row so that the comparator's unfilter step is a reshape (its pure-Python unfilter
would dominate); zlib's inflate stays in the comparator, as libpng's does in the reference.

    python tools/gt_read_time.py --dataset u4k [--runs 9] [--out profiles/gt_read_time.jsonl]
One dataset per process: run them one after the other.
"""
import argparse
import json
import os
import sys
import time
import zlib

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NATIVE = {"u4k": (2160, 3840), "eth3d": (4032, 6048), "mid": (1988, 2964), "gta": (1080, 1920), "cityscapes": (1024, 2048)}
SPEC_GBPS = 8000.0


def scene(H, W, lo, hi):
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    u = 0.5 + 0.3 * np.sin(xx / 160) * np.cos(yy / 120) + 0.15 * (xx > W // 2) + 0.02 * np.random.RandomState(0).rand(H, W).astype(np.float32)
    return (lo + (hi - lo) * np.clip(u, 0, 1)).astype(np.float32)


def png16_filter0(samples, P):
    H, W = samples.shape
    rows = np.zeros((H, 1 + 2 * W), np.uint8)
    rows[:, 1:] = samples.astype(">u2").view(np.uint8).reshape(H, 2 * W)
    return P.write_png(samples, 0, 16, filtered=rows.tobytes())


def fast_decode(P):
    def decode(png):
        h = P.parse(png)
        raw = np.frombuffer(zlib.decompress(h["idat"]), np.uint8).reshape(h["height"], 1 + h["rowbytes"])
        assert h["depth"] == 16 and h["color_type"] == 0 and not raw[:, 0].any()
        return raw[:, 1:].reshape(h["height"], h["width"], 2).view(">u2")[..., 0].astype(np.uint16)
    return decode


def make_file(dataset, R):
    H, W = NATIVE[dataset]
    if dataset == "u4k":
        return R.npy_bytes(scene(H, W, 20.0, 400.0)), dict(depth_factor=1832.4375)
    if dataset == "mid":
        x = scene(H, W, 30.0, 260.0)
        x[::97, ::89] = np.inf                                        # Middlebury marks unknown disparities with inf
        return R.pfm_bytes(x, True), dict(calib=R.CALIB)
    if dataset == "eth3d":
        x = scene(H, W, 1.0, 40.0)
        x[::5, ::3] = np.inf                                          # ETH3D's depth maps are sparse: inf where nothing was measured
        return x.astype("<f4").tobytes(), dict(shape=(H, W))
    if dataset == "gta":
        return png16_filter0((scene(H, W, 2.0, 200.0) * 256).astype(np.uint16), R.P), {}
    return png16_filter0((scene(H, W, 2.0, 120.0) * 256 + 1).astype(np.uint16), R.P), {}


def median_ms(v):
    return round(float(np.median(v)) * 1e3, 3)


def dev_time_us(fn, iters=30, warmup=3):
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
    ap.add_argument("--dataset", required=True, choices=sorted(NATIVE))
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gt_read_time.jsonl"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    assert args.runs >= 9
    from patchfusion_amd import groundtruth as gt
    from patchfusion_amd.hip_ops import ops
    from tests import gt_ref as R

    ds = args.dataset
    H, W = NATIVE[ds]
    data, kw = make_file(ds, R)
    if ds in ("gta", "cityscapes"):
        R.P.decode = fast_decode(R.P)

    def device_reader():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        g = gt.read_depth_gt(data, ds, **kw)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, g

    def comparator():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        depth, _, edge = R.depth_map(ds, data, **kw)
        t1 = time.perf_counter()
        d, e = torch.from_numpy(depth).cuda(), torch.from_numpy(edge).cuda()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, t1 - t0, (depth, edge, d, e)

    _, g = device_reader()
    _, _, (depth, edge, _, _) = comparator()
    assert R.same_bits(g.depth.cpu().numpy(), depth) and R.same_bits(g.edge.cpu().numpy(), edge), "device and host planes differ"
    ta, tb, tb_host = [], [], []
    for _ in range(args.runs):
        ta.append(device_reader()[0])
        t, th, _ = comparator()
        tb.append(t)
        tb_host.append(th)

    # the parts of the new path
    info = g.info
    res = {"dataset": ds, "grid": [H, W], "device": torch.cuda.get_device_name(0), "runs": args.runs, "file_bytes": len(data),
           "format": info.format, "dtype": info.dtype, "bytes_uploaded": int(info.bytes_uploaded), "verified_bit_exact": True,
           "device_reader_ms_median": median_ms(ta), "device_reader_ms_min_max": [round(min(ta) * 1e3, 3), round(max(ta) * 1e3, 3)],
           "host_comparator_ms_median": median_ms(tb), "host_comparator_ms_min_max": [round(min(tb) * 1e3, 3), round(max(tb) * 1e3, 3)],
           "host_comparator_numpy_ms_median": median_ms(tb_host), "note": "measured on one box"}
    res["device_reader_faster"] = bool(res["device_reader_ms_median"] < res["host_comparator_ms_median"])
    if info.format == "png":
        from patchfusion_amd.preprocess import decode_png
        res["png_inflate"] = info.png.inflate
        ts = []
        for _ in range(args.runs):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            src, _ = decode_png(data)
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        res["decode_png_ms_median"] = median_ms(ts)                  # upload + inflate + unfilter + expand
        kind, mode, own_edge, sample = info.dtype, ds, False, 2
    else:
        off = len(data) - info.bytes_uploaded
        ts = []
        for _ in range(args.runs):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            src = gt._upload(data, off, info.bytes_uploaded, torch.device("cuda"))
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        res["upload_ms_median"] = median_ms(ts)
        res["upload_GBps"] = round(info.bytes_uploaded / float(np.median(ts)) / 1e9, 2)
        kind, mode, own_edge, sample = "f4", ds, ds in ("u4k", "mid"), 4
    a, b = {"u4k": (kw.get("depth_factor", 0), 0), "mid": (R.CALIB[2] * R.CALIB[0], R.CALIB[1]), "cityscapes": (gt.CITYSCAPES_FACTOR, 0)}.get(ds, (0, 0))
    d = torch.empty(H, W, dtype=torch.float32, device="cuda")
    e = torch.empty_like(d) if own_edge else None
    out = torch.empty_like(d)
    us = dev_time_us(lambda: ops.gt_convert(src, kind, mode, H, W, a, b, d, e, flip=ds == "mid"))
    nbytes = H * W * (sample + 4 + (4 if own_edge else 0))
    res["convert_kernel"] = {"us": round(us, 2), "algorithmic_bytes": nbytes, "GBps": round(nbytes / us / 1e3, 1),
                             "share_of_8TBps_spec": round(nbytes / us / 1e3 / SPEC_GBPS, 3)}
    us_b = dev_time_us(lambda: ops.depth_boundaries(e if own_edge else d, 1.0, 0, out))
    res["boundary_kernel"] = {"us": round(us_b, 2), "algorithmic_bytes": 8 * H * W, "GBps": round(8 * H * W / us_b / 1e3, 1)}
    res["device_kernels_ms"] = round((us + us_b) / 1e3, 4)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(res) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
