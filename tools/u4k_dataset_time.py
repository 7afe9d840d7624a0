"""Times datasets.UnrealStereo4kDataset.__getitem__('train') at 2160 x 3840 on the device against the host path it replaces -- the
restatement of tests/u4k_aug_ref.py (host_sample: Pillow, numpy and torch on the CPU, the reference's operations in its order) followed by
the upload of its tensors -- on the same synthetic files, with the same draws, interleaved in one process, and writes
profiles/u4k_dataset_time.json:

  * whole sample: wall clock from the files on disk to tensors on the device, a device synchronisation before and after; one warm-up of
    each path, then the median, minimum and maximum of --runs (>= 20) runs; the host path runs with at most --threads (16) threads;
  * per stage of each path (upload, ground-truth conversion, planes, image, resizes): the device path in a second run per draw with
    dataset.timing (every stage ended by a synchronise, so the stages sum to more than the untimed sample), the host path with
    host_sample's own stage clock in the timed run itself; medians over the runs.  The files are read from the page cache by both
    paths: file reading is inside "whole sample" and outside the stages.
Before anything is timed the device sample is compared with the host sample: depth, crop and box bit for bit, the images within 2^-21.

    python tools/u4k_dataset_time.py [--runs 20] [--out profiles/u4k_dataset_time.json]
"""
import argparse
import json
import os
import random
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

IMAGE, PATCH, NET = (2160, 3840), (540, 960), (384, 512)
STAGES = ("upload", "ground_truth", "planes", "image", "resizes")


def summary(values):
    ms = [1e3 * v for v in values]
    return dict(median_ms=round(statistics.median(ms), 3), min_ms=round(min(ms), 3), max_ms=round(max(ms), 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "u4k_dataset_time.json"))
    args = ap.parse_args()
    assert args.runs >= 20 and torch.cuda.is_available(), "a measurement needs a GPU and at least 20 runs"
    torch.set_num_threads(min(args.threads, 16))
    from patchfusion_amd.datasets import UnrealStereo4kDataset
    from tests import u4k_aug_ref as R
    dev = torch.device("cuda")
    with tempfile.TemporaryDirectory() as root:
        split, _ = R.write_root(root, IMAGE, n=1, seed=1)
        ds = UnrealStereo4kDataset("train", root, split, dict(degree=1.0, random_crop=True, network_process_size=list(NET)), 1e-3, 80,
                                   patch_raw_shape=PATCH, device=dev, image_shape=IMAGE)
        info = ds.data_infos[0]

        def host(seed, stages=None):
            random.seed(seed)
            np.random.seed(seed)
            d = R.draw(1.0, IMAGE, PATCH)
            img = np.fromfile(info["img_path"], dtype=np.uint8).reshape(IMAGE + (3,))
            disp = np.load(info["depth_map_path"])
            s = R.host_sample(img, disp, info["depth_factor"], d, PATCH, NET, stages)
            t0 = time.perf_counter()
            out = {k: s[k].to(dev) for k in ("image_lr", "crops_image_hr", "depth_gt", "crop_depths", "bboxs")}
            torch.cuda.synchronize()
            if stages is not None:
                stages["upload"] = time.perf_counter() - t0
            return out, d

        def device(seed, stages=None):
            random.seed(seed)
            np.random.seed(seed)
            ds.timing = stages
            return ds[0]

        def timed(fn, seed, stages=None):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn(seed, stages)
            torch.cuda.synchronize()
            return time.perf_counter() - t0, out

        (want, d), got = host(0), device(0)                                        # warm-up of both, and the comparison
        for k in ("depth_gt", "crop_depths", "bboxs"):
            assert torch.equal(want[k], got[k]), k
        for k in ("image_lr", "crops_image_hr"):
            assert float((want[k] - got[k]).abs().max()) <= 2.0 ** -21, k
        whole = {"device": [], "host": []}
        stage = {"device": {k: [] for k in STAGES}, "host": {k: [] for k in STAGES}}
        fired = 0
        for i in range(args.runs):
            whole["device"].append(timed(device, 100 + i)[0])
            st = {}
            timed(device, 100 + i, st)                                             # the staged run synchronises per stage: timed apart
            for k in STAGES:
                stage["device"][k].append(st.get(k, 0.0))
            st = {}
            whole["host"].append(timed(host, 100 + i, st)[0])                      # the host's stage clock adds no synchronisation
            for k in STAGES:
                stage["host"][k].append(st.get(k, 0.0))
            random.seed(100 + i)
            random.random()
            fired += random.random() > 0.5
        ds.timing = None
    result = dict(tool="tools/u4k_dataset_time.py", device=torch.cuda.get_device_name(0), image=list(IMAGE), patch=list(PATCH), network=list(NET),
                  runs=args.runs, host_threads=torch.get_num_threads(), colour_augmentation_fired=f"{fired} of {args.runs} runs",
                  whole_sample={k: summary(v) for k, v in whole.items()},
                  stages={n: {k: summary(v) for k, v in stage[n].items()} for n in stage})
    result["whole_sample"]["host_over_device"] = round(result["whole_sample"]["host"]["median_ms"] / result["whole_sample"]["device"]["median_ms"], 2)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
