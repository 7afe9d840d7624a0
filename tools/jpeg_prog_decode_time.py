"""Times preprocess.decode_jpeg(..., progressive=True) against the host decode it replaces (PIL + upload of the array), on one GPU, by
the method of tools/jpeg_decode_time.py, and writes profiles/jpeg_prog_decode_time.json.  Inputs: that tool's seeded photo-like images
encoded here by PIL at q90, progressive, 4:2:0: 2300x1586, 3840x2160 and 6048x4032.  The arms (PIL + upload, entropy='host',
entropy='device' at each --bits) alternate in one process after every arm was warmed and checked against PIL; each timing ends in a
device synchronise.  A further pass per file splits the device arm at the default subsequence length into its parts (each part ending in
a synchronise of its own, so their sum exceeds the arm's time) and records the rounds of every scan.
    python tools/jpeg_prog_decode_time.py [--reps 7] [--bits 256 1024 4096] [--out profiles/jpeg_prog_decode_time.json]"""
import argparse
import io
import json
import os
import sys

import numpy as np
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from patchfusion_amd import preprocess as P  # noqa: E402
from tools.jpeg_decode_time import photo, timed  # noqa: E402


def encode(a):
    buf = io.BytesIO()
    Image.fromarray(a).save(buf, "JPEG", quality=90, progressive=True, subsampling="4:2:0")
    return buf.getvalue()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--bits", type=int, nargs="+", default=[256, 1024, 4096])
    ap.add_argument("--only", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpeg_prog_decode_time.json"))
    args = ap.parse_args()
    from patchfusion_amd.hip_ops import ops
    shapes = {"2300x1586_420": (1586, 2300, 1), "3840x2160_420": (2160, 3840, 2), "6048x4032_420": (4032, 6048, 3)}
    if args.only:
        shapes = {args.only: shapes[args.only]}
    out = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "files": {}}
    for name, (H, W, seed) in shapes.items():
        data = encode(photo(H, W, seed))
        arms = {"pil_upload": lambda: torch.from_numpy(np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))).cuda(),
                "host_entropy": lambda: P.decode_jpeg(data, entropy="host", progressive=True)}
        for S in args.bits:
            arms[f"device_entropy_S{S}"] = lambda S=S: P.decode_jpeg(data, entropy="device", subsequence_bits=S, max_sync_rounds=1 << 20, progressive=True)
        ref = arms["pil_upload"]()
        host = P.JpegProgHost(data)
        kinds = [P.JPEG_PROG_KINDS[s.kind] for s in host.scans]
        rec = {"jpeg_bytes": len(data), "rgb_bytes": int(ref.numel()), "scans": len(host.scans),
               "entropy_bytes_by_kind": {k: int(sum(s.end - s.begin for s in host.scans if P.JPEG_PROG_KINDS[s.kind] == k)) for k in sorted(set(kinds))},
               "arms": {}}
        for k, fn in arms.items():                                         # warm every arm and check it
            r = fn()
            if k != "pil_upload":
                assert torch.equal(r[0], ref), (name, k)
                rec["arms"][k] = {"entropy_used": r[1].entropy, "sync_rounds": r[1].sync_rounds, "bytes_uploaded": r[1].bytes_uploaded,
                                  "bytes_downloaded": getattr(r[1], "bytes_downloaded", 0),
                                  "rounds_per_scan": [(e["kind"], e["sync_rounds"]) for e in r[1].scans if e["decoded"] == "device"]}
            else:
                rec["arms"][k] = {"bytes_uploaded": int(ref.numel())}
        ts = {k: [] for k in arms}
        for _ in range(args.reps):                                         # alternate the arms
            for k, fn in arms.items():
                ts[k] += timed(fn, 1)
        for k in arms:
            rec["arms"][k].update(ms_median=float(np.median(ts[k])), ms_min=float(min(ts[k])), ms_max=float(max(ts[k])))
        parts = []
        for _ in range(args.reps):                                         # the split of the device arm's entropy step
            t = {}
            rc = P.jpeg_prog_entropy_device(host, ops, torch.device("cuda"), P.JPEG_SUBSEQUENCE_BITS, 1 << 20, timing=t)[0]
            assert rc == 0
            parts.append(t)
        rec["device_split_ms"] = {"subsequence_bits": P.JPEG_SUBSEQUENCE_BITS,
                                  **{k: {"median": float(np.median([p[k] for p in parts]) * 1e3), "min": float(min(p[k] for p in parts) * 1e3),
                                         "max": float(max(p[k] for p in parts) * 1e3)} for k in sorted(parts[0])}}
        out["files"][name] = rec
        print(name, {k: round(v["ms_median"], 2) for k, v in rec["arms"].items()}, {k: round(v["median"], 2) for k, v in rec["device_split_ms"].items() if k != "subsequence_bits"}, flush=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
