"""Writes tests/golden/u4k_aug_small.npz: small inputs, seeds and what the REFERENCE's own aug_rotate / aug_color / aug_flip / random_crop
(estimator/datasets/transformers/augmentations.py, through oracle.ref_shim) make of them in the order of UnrealStereo4kDataset.__getitem__
(u4k_dataset.py:118-151), so that tests/test_u4k_aug_ref_cpu.py can hold the restatement of tests/u4k_aug_ref.py to the reference where
the reference's tree is absent.  Run from the repository root in the build container:  python tests/make_u4k_aug_golden.py"""
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPE, CROP, DEGREES, SEEDS = (37, 53), (16, 24), (1.0, 5.0), (0, 1, 4, 7)       # the seeds: colour and flip on / off in all four pairings


def reference_sample(aug, image, disp, depth_factor, degree, seed):
    """the train branch of u4k_dataset.py:118-151 on arrays, with the reference's functions; -> dict of arrays"""
    import torch
    random.seed(seed)
    np.random.seed(seed)
    disp_gt = disp.astype(np.float32)
    depth_gt = depth_factor / disp_gt
    rot, (depth_gt, disp_gt) = aug.aug_rotate(image, [depth_gt, disp_gt], degree)
    unit = rot.astype(np.float32)[:, :, ::-1].copy() / 255.0
    col = aug.aug_color(unit)
    out, (depth_gt, disp_gt) = aug.aug_flip(col, [depth_gt, disp_gt])
    t = torch.from_numpy(np.ascontiguousarray(out.transpose(2, 0, 1)))
    _, (crop_depth, _), (h0, w0) = aug.random_crop(t, [torch.from_numpy(depth_gt[None].copy()), torch.from_numpy(disp_gt[None].copy())], CROP)
    return dict(rotated=rot, coloured=bool(col is not unit), image=np.ascontiguousarray(out, dtype=np.float32), depth=np.ascontiguousarray(depth_gt),
                crop_depth=crop_depth.numpy(), start=np.array([h0, w0]),
                after=np.array([random.random(), np.random.random()]))


def main():
    from oracle import ref_shim
    ref_shim.import_reference()
    from estimator.datasets.transformers import augmentations as aug
    rng = np.random.default_rng(20240)
    H, W = SHAPE
    out = dict(shape=np.array(SHAPE), crop=np.array(CROP), seeds=np.array(SEEDS), degrees=np.array(DEGREES),
               image=rng.integers(0, 256, (H, W, 3), dtype=np.uint8), disp=(rng.random((H, W), dtype=np.float32) * 180 + 2).astype(np.float32),
               depth_factor=np.array(37.75 * 1109.25))
    seen = set()
    for degree in DEGREES:
        for seed in SEEDS:
            r = reference_sample(aug, out["image"], out["disp"], float(out["depth_factor"]), degree, seed)
            seen.add(r["coloured"])
            for k, v in r.items():
                out[f"d{degree:g}_s{seed}_{k}"] = np.asarray(v)
    assert seen == {True, False}, "the seeds cover the colour augmentation on and off"
    path = os.path.join(ROOT, "tests", "golden", "u4k_aug_small.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
