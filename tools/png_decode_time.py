"""Times preprocess.decode_png against the host decode it replaces (PIL + upload of the array), on one GPU, and writes
profiles/png_decode_time.json.  Inputs: the seeded photo-like images of tools/jpeg_decode_time.py at 2048x1024 and 3840x2160, written by
PIL as RGB8 at compress levels 6 and 1, a 16-bit grey plane at both sizes, and one save_prediction pair at 1568x2072.  The three arms
(PIL + upload, inflate='host', inflate='device') alternate in one process after every file was warmed and checked; each timing ends in a
device synchronise.  A separate pass (timing=, a synchronise after every stage) splits the device arm into finder, scan, chain walk with
its copies, inflate, resolve, Adler, unfilter + expand.
    python tools/png_decode_time.py [--reps 7] [--only NAME] [--out profiles/png_decode_time.json]
--subsequences times the opt-in block_decode='subsequences' instead: the arms are inflate='host', inflate='device' (sequential) and the new
mode at lanes of 128, 256, 512 and 1024 bits, alternated in the same way; the per-stage split is taken for every device arm, and the
results go to profiles/png_inflate_par_time.json, so that the file above stays as it was measured.  The workgroup size is a constant of
the library (PF_PNGD_PAR_WINDOW); to time another one, build a variant (make -C patchfusion_amd/csrc variant NAME=.. DEFS=-DPF_PNGD_PAR_WINDOW=..),
load it with PF_LIB_PATH and give --out another name.
    python tools/png_decode_time.py --subsequences [--reps 7] [--only NAME] [--out profiles/png_inflate_par_time.json]"""
import argparse
import io
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from patchfusion_amd import postprocess  # noqa: E402
from patchfusion_amd.preprocess import decode_png  # noqa: E402
from tools.jpeg_decode_time import photo  # noqa: E402


def encode(a, level):
    buf = io.BytesIO()
    Image.fromarray(a).save(buf, "PNG", compress_level=level)
    return buf.getvalue()


def grey16(H, W, seed):
    a = photo(H, W, seed).astype(np.float64)
    v = a[..., 0] * 200.0 + a[..., 1] * 50.0 + np.random.default_rng(seed).normal(0, 40, (H, W))
    return np.clip(v, 0, 65535).astype(np.uint16)


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def pil_upload(data):
    im = Image.open(io.BytesIO(data))
    if im.mode in ("I;16", "I"):
        return torch.from_numpy(np.asarray(im).astype(np.uint16)).cuda()
    return torch.from_numpy(np.asarray(im.convert("RGB"))).cuda()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--only", default=None, help="time this one file only")
    ap.add_argument("--subsequences", action="store_true", help="time block_decode='subsequences' against the host and the sequential device arm")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "png_inflate_par_time.json" if args.subsequences else "png_decode_time.json")
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    files = {}
    for (H, W), seed in (((1024, 2048), 1), ((2160, 3840), 2)):
        rgb = photo(H, W, seed)
        files[f"{W}x{H}_rgb8_l6"] = encode(rgb, 6)
        files[f"{W}x{H}_rgb8_l1"] = encode(rgb, 1)
        files[f"{W}x{H}_grey16_l6"] = encode(grey16(H, W, seed), 6)
    depth = torch.from_numpy(photo(1568, 2072, 5)[..., 0].astype(np.float32) / 255.0 * 9.0 + 0.5).cuda()
    with tempfile.TemporaryDirectory() as d:
        for path, name in zip(postprocess.save_prediction(depth[None, None], d, "pred"), ("save_prediction_2072x1568_colour", "save_prediction_2072x1568_uint16")):
            with open(path, "rb") as f:
                files[name] = f.read()
    if args.only:
        files = {args.only: files[args.only]}
    out = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "files": {}}
    if args.subsequences:
        return subsequences(files, args, out)
    for name, data in files.items():
        arms = {"pil_upload": lambda: pil_upload(data), "host_inflate": lambda: decode_png(data, inflate="host"),
                "device_inflate": lambda: decode_png(data, inflate="device")}
        ref = arms["pil_upload"]()
        rec = {"png_bytes": len(data), "image_bytes": int(ref.numel() * ref.element_size()), "arms": {}}
        for k, fn in arms.items():                                         # warm every arm and check it
            r = fn()
            if k != "pil_upload":
                assert r[0].dtype == ref.dtype and torch.equal(r[0], ref), (name, k)
                i = r[1]
                rec["arms"][k] = {"inflate_used": i.inflate, "fallback_reason": i.fallback_reason, "blocks": i.blocks, "candidates": i.candidates,
                                  "chain_rounds": i.chain_rounds, "resolve_rounds": i.resolve_rounds, "bytes_uploaded": i.bytes_uploaded,
                                  "bytes_downloaded": i.bytes_downloaded}
            else:
                rec["arms"][k] = {"bytes_uploaded": rec["image_bytes"]}
        ts = {k: [] for k in arms}
        for _ in range(args.reps):                                         # alternate the arms
            for k, fn in arms.items():
                ts[k].append(timed(fn))
        for k in arms:
            rec["arms"][k].update(ms_median=float(np.median(ts[k])), ms_min=float(min(ts[k])), ms_max=float(max(ts[k])))
        stages = []
        for _ in range(3):                                                 # the per-stage split: its own pass, a synchronise per stage
            t = {}
            decode_png(data, inflate="device", timing=t)
            stages.append(t)
        rec["device_stages_ms"] = {k: float(np.median([s.get(k, 0.0) for s in stages])) * 1e3 for k in stages[0]}
        stages = []
        for _ in range(3):
            t = {}
            decode_png(data, inflate="host", timing=t)
            stages.append(t)
        rec["host_stages_ms"] = {k: float(np.median([s.get(k, 0.0) for s in stages])) * 1e3 for k in stages[0]}
        out["files"][name] = rec
        print(name, {k: round(v["ms_median"], 2) for k, v in rec["arms"].items()}, {k: round(v, 2) for k, v in rec["device_stages_ms"].items()}, flush=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", args.out)


LANE_BITS = (128, 256, 512, 1024)


def subsequences(files, args, out):
    from patchfusion_amd import _lib
    out["window_threads"] = _lib.load().pf_pngd_par_window()
    out["lane_bits"] = list(LANE_BITS)
    for name, data in files.items():
        arms = {"host_inflate": dict(inflate="host"), "device_sequential": dict(inflate="device")}
        for bits in LANE_BITS:
            arms[f"device_subsequences_{bits}"] = dict(inflate="device", block_decode="subsequences", subsequence_bits=bits)
        ref = pil_upload(data)
        rec = {"png_bytes": len(data), "image_bytes": int(ref.numel() * ref.element_size()), "arms": {}}
        for k, kw in arms.items():                                         # warm every arm and check it
            img, i = decode_png(data, **kw)
            assert img.dtype == ref.dtype and torch.equal(img, ref), (name, k)
            assert i.inflate == kw["inflate"] and i.fallback_reason is None, (name, k, i)
            rec["arms"][k] = {"inflate_used": i.inflate, "block_decode": i.block_decode, "sync_rounds": i.sync_rounds, "blocks": i.blocks,
                              "candidates": i.candidates, "chain_rounds": i.chain_rounds, "resolve_rounds": i.resolve_rounds}
        ts = {k: [] for k in arms}
        for _ in range(args.reps):                                         # alternate the arms
            for k, kw in arms.items():
                ts[k].append(timed(lambda: decode_png(data, **kw)))
        for k in arms:
            rec["arms"][k].update(ms_median=float(np.median(ts[k])), ms_min=float(min(ts[k])), ms_max=float(max(ts[k])))
        for k, kw in arms.items():                                         # the per-stage split: its own pass, a synchronise per stage
            stages = []
            for _ in range(args.reps):
                t = {}
                decode_png(data, timing=t, **kw)
                stages.append(t)
            rec["arms"][k]["stages_ms"] = {s: float(np.median([x.get(s, 0.0) for x in stages])) * 1e3 for s in stages[0]}
            if kw["inflate"] == "device":
                both = [(x["scan"] + x["inflate"]) * 1e3 for x in stages]
                rec["arms"][k].update(scan_inflate_ms_median=float(np.median(both)), scan_inflate_ms_min=float(min(both)), scan_inflate_ms_max=float(max(both)))
        out["files"][name] = rec
        print(name, {k: (round(v["ms_median"], 2), round(v.get("scan_inflate_ms_median", 0.0), 2), v["sync_rounds"]) for k, v in rec["arms"].items()}, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
