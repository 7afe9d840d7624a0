"""Times preprocess.decode_jpeg against the host decode it replaces (PIL + upload of the array), on one GPU, and writes
profiles/jpeg_decode_time.json.  Inputs: seeded photo-like images (smooth + edges + noise) encoded here by PIL at q90: 2300x1586,
3840x2160 and 6048x4032 at 4:2:0, 3840x2160 also at 4:4:4 and with a restart interval of one MCU row.  The three arms (PIL + upload,
entropy='device', entropy='host') alternate in one process after every shape was warmed; each timing ends in a device synchronise.
Per-kernel times come from a separate `rocprofv3 --kernel-trace --stats --output-format csv -- python tools/jpeg_decode_time.py --only
3840x2160_420 --bits 1024 --reps 2` run, merged with --merge-kernel-stats <kernel_stats.csv>.
    python tools/jpeg_decode_time.py [--reps 7] [--bits 1024] [--out profiles/jpeg_decode_time.json]"""
import argparse
import io
import json
import os
import re
import sys
import time

import numpy as np
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from patchfusion_amd.preprocess import decode_jpeg  # noqa: E402


def photo(H, W, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    a = np.stack([127 + 80 * np.sin(xx / (90 + 30 * c)) * np.cos(yy / (70 + 20 * c)) for c in range(3)], axis=-1)
    for _ in range(40):                                                    # rectangles: hard edges
        y0, x0 = int(rng.integers(0, H)), int(rng.integers(0, W))
        a[y0:y0 + int(rng.integers(20, H // 3)), x0:x0 + int(rng.integers(20, W // 3))] += rng.uniform(-60, 60, 3)
    a += rng.normal(0, 6, a.shape)                                         # sensor noise
    return np.clip(a, 0, 255).astype(np.uint8)


def encode(a, **kw):
    buf = io.BytesIO()
    Image.fromarray(a).save(buf, "JPEG", quality=90, **kw)
    return buf.getvalue()


def timed(fn, reps):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t) * 1e3)
    return ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--bits", type=int, nargs="+", default=[256, 1024, 4096])
    ap.add_argument("--only", default=None, help="time this one file only (the rocprofv3 run)")
    ap.add_argument("--merge-kernel-stats", default=None, help="rocprofv3 kernel_stats.csv of a --only run: add its jpeg_* rows to --out and exit")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpeg_decode_time.json"))
    args = ap.parse_args()
    if args.merge_kernel_stats:
        import csv
        with open(args.out) as f:
            out = json.load(f)
        rows = [r for r in csv.DictReader(open(args.merge_kernel_stats)) if "jpeg_" in r["Name"]]
        out["kernel_trace"] = {"file": args.only, "note": "separate rocprofv3 --kernel-trace --stats run; all arms of that file, warm-up included",
                               "kernels": {re.search(r"jpeg_\w+", r["Name"]).group(0): {"calls": int(r["Calls"]), "total_us": float(r["TotalDurationNs"]) / 1e3,
                                                                      "avg_us": float(r["AverageNs"]) / 1e3} for r in rows}}
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
        return
    files = {"2300x1586_420": encode(photo(1586, 2300, 1), subsampling="4:2:0"), "3840x2160_420": encode(photo(2160, 3840, 2), subsampling="4:2:0"),
             "6048x4032_420": encode(photo(4032, 6048, 3), subsampling="4:2:0"), "3840x2160_444": encode(photo(2160, 3840, 2), subsampling="4:4:4"),
             "3840x2160_420_rst": encode(photo(2160, 3840, 2), subsampling="4:2:0", restart_marker_rows=1)}
    if args.only:
        files = {args.only: files[args.only]}
    out = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "files": {}}
    for name, data in files.items():
        arms = {"pil_upload": lambda: torch.from_numpy(np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))).cuda(),
                "host_entropy": lambda: decode_jpeg(data, entropy="host")}
        for S in args.bits:
            arms[f"device_entropy_S{S}"] = lambda S=S: decode_jpeg(data, entropy="device", subsequence_bits=S, max_sync_rounds=1 << 20)
        ref = arms["pil_upload"]()
        rec = {"jpeg_bytes": len(data), "rgb_bytes": int(ref.numel()), "arms": {}}
        for k, fn in arms.items():                                         # warm every arm and check it
            r = fn()
            if k != "pil_upload":
                assert torch.equal(r[0], ref), (name, k)
                rec["arms"][k] = {"entropy_used": r[1].entropy, "sync_rounds": r[1].sync_rounds, "bytes_uploaded": r[1].bytes_uploaded}
            else:
                rec["arms"][k] = {"bytes_uploaded": int(ref.numel())}
        ts = {k: [] for k in arms}
        for _ in range(args.reps):                                         # alternate the arms
            for k, fn in arms.items():
                ts[k] += timed(fn, 1)
        for k in arms:
            rec["arms"][k].update(ms_median=float(np.median(ts[k])), ms_min=float(min(ts[k])), ms_max=float(max(ts[k])))
        out["files"][name] = rec
        print(name, {k: round(v["ms_median"], 2) for k, v in rec["arms"].items()}, flush=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
