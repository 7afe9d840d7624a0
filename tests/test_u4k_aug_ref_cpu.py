"""tests/u4k_aug_ref.py -- the numpy restatement the GPU tests of csrc/augment.hip compare against -- held to its three authorities on the
CPU: Pillow itself (exact), the reference's own augmentations and UnrealStereo4kDataset.__getitem__ (exact except downstream of `**gamma`,
where numpy's float32 power may differ between builds; generator states equal), and a committed fixture of the reference's outputs
(tests/make_u4k_aug_golden.py) for where the reference's tree is absent."""
import os
import random

import numpy as np
import pytest

from tests import u4k_aug_ref as R

# downstream of `**`: numpy's float32 power is within one ulp (2^-23 relative) of the exact power, the two products add one rounding each
POW_BAR = 2.0 ** -23 + 2 * 2.0 ** -24
SIZES = [(37, 53), (64, 96)]


def angles(degree_list=(1.0, 5.0)):
    rng = random.Random(11)
    out = [0.0, 1e-3]
    for degree in degree_list:
        out += [degree, -degree] + [(rng.random() - 0.5) * 2 * degree for _ in range(3)]
    return out


def inputs(H, W, seed=0):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (H, W, 3), dtype=np.uint8), (rng.random((H, W), dtype=np.float32) * 180 + 2).astype(np.float32)


def pillow(img, plane, angle):
    Image = pytest.importorskip("PIL.Image")
    return (np.asarray(Image.fromarray(img).rotate(angle, resample=Image.BILINEAR)),
            np.asarray(Image.fromarray(plane).rotate(angle, resample=Image.NEAREST)))


@pytest.mark.parametrize("H,W", SIZES)
def test_rotations_equal_pillow(H, W):
    pytest.importorskip("PIL")
    img, plane = inputs(H, W)
    for angle in angles():
        m = R.rotate_matrix(angle, W, H)
        want_img, want_plane = pillow(img, plane, angle)
        assert np.array_equal(R.rotate_image_bilinear(img, m), want_img), angle
        assert np.array_equal(R.rotate_plane_nearest(plane, R.fix16(m)), want_plane), angle
        assert np.array_equal(R.rotate_image_bilinear(img, m, flip=True), want_img[:, ::-1]), angle
        assert np.array_equal(R.rotate_plane_nearest(plane, R.fix16(m), flip=True), want_plane[:, ::-1]), angle


def test_rotations_equal_pillow_at_full_size():
    """2160 x 3840: the only size at which the 16.16 sums and the double coordinates reach their working range"""
    pytest.importorskip("PIL")
    H, W = 2160, 3840
    img, plane = inputs(H, W, 3)
    angle = -0.8731
    m = R.rotate_matrix(angle, W, H)
    want_img, want_plane = pillow(img, plane, angle)
    assert np.array_equal(R.rotate_image_bilinear(img, m), want_img)
    assert np.array_equal(R.rotate_plane_nearest(plane, R.fix16(m)), want_plane)


def test_unit_image_is_one_float32_division_for_every_byte():
    """the validation path divides in double and rounds (ImagePreprocessor), the reference's u4k dataset divides in float32: the same 256 values"""
    b = np.arange(256, dtype=np.uint8)
    assert np.array_equal((b / 255.0).astype(np.float32), b.astype(np.float32) / 255.0)


def restated(img, disp, depth_factor, degree, crop, seed):
    """the restatement of the train branch with its own draws -> the keys of tests/make_u4k_aug_golden.reference_sample"""
    random.seed(seed)
    np.random.seed(seed)
    H, W = disp.shape
    d = R.draw(degree, (H, W), crop)
    m = R.rotate_matrix(d["angle"], W, H)
    depth = R.rotate_plane_nearest((np.float32(depth_factor) / disp.astype(np.float32)).astype(np.float32), R.fix16(m), d["flip"])
    unit = R.to_unit_f32(R.rotate_image_bilinear(img, m, d["flip"]))
    h0, w0 = d["h0"], d["w0"]
    return d, dict(rotated=R.rotate_image_bilinear(img, m), image32=R.colour_f32(unit, d), image64=R.colour_f64(unit, d)[0], depth=depth,
                   crop_depth=depth[None, h0:h0 + crop[0], w0:w0 + crop[1]], start=np.array([h0, w0]),
                   after=np.array([random.random(), np.random.random()]))


def check_against(want, d, got):
    assert np.array_equal(got["rotated"], want["rotated"])
    assert bool(want["coloured"]) == d["colour"]
    assert np.array_equal(got["depth"], want["depth"]) and np.array_equal(got["crop_depth"], want["crop_depth"])
    assert np.array_equal(got["start"], want["start"])
    assert np.array_equal(got["after"], want["after"]), "the generators are left in the reference's state"
    if d["colour"]:
        err = np.abs(want["image"].astype(np.float64) - got["image64"])
        assert (err <= POW_BAR * np.abs(got["image64"]) + 1e-45).all(), float((err / (np.abs(got["image64"]) + 1e-30)).max())
    else:
        assert np.array_equal(got["image32"], want["image"])


def test_restatement_equals_the_committed_reference_outputs(golden_dir):
    g = np.load(os.path.join(golden_dir, "u4k_aug_small.npz"))
    seen = set()
    for degree in g["degrees"].tolist():
        for seed in g["seeds"].tolist():
            d, got = restated(g["image"], g["disp"], float(g["depth_factor"]), degree, tuple(g["crop"].tolist()), seed)
            check_against({k: g[f"d{degree:g}_s{seed}_{k}"] for k in ("rotated", "coloured", "image", "depth", "crop_depth", "start", "after")}, d, got)
            seen.add((d["colour"], d["flip"]))
    assert len(seen) == 4


@pytest.mark.reference
def test_restatement_equals_the_reference_functions():
    from oracle import ref_shim
    if not ref_shim.reference_available():
        pytest.skip("reference tree not present")
    pytest.importorskip("PIL")
    ref_shim.import_reference()
    from estimator.datasets.transformers import augmentations as aug
    from tests.make_u4k_aug_golden import CROP, reference_sample
    for (H, W), degree, seed in (((37, 53), 1.0, 0), ((37, 53), 5.0, 4), ((64, 96), 5.0, 1), ((64, 96), 1.0, 7)):
        img, disp = inputs(H, W, seed)
        want = reference_sample(aug, img, disp, 41881.5, degree, seed)
        d, got = restated(img, disp, 41881.5, degree, CROP, seed)
        check_against(want, d, got)


@pytest.mark.reference
@pytest.mark.parametrize("mode,seed", [("train", 0), ("train", 4), ("infer", 0)])
def test_restatement_equals_the_reference_dataset_at_full_size(tmp_path, mode, seed):
    """the reference's UnrealStereo4kDataset.__getitem__ on a synthetic root of one 2160 x 3840 sample, both modes"""
    from oracle import ref_shim
    if not ref_shim.reference_available():
        pytest.skip("reference tree not present")
    pytest.importorskip("PIL")
    import torch
    ref_shim.import_reference()
    from estimator.datasets.u4k_dataset import UnrealStereo4kDataset as RefDataset
    H, W, crop, net = 2160, 3840, (540, 960), (384, 512)
    split, samples = R.write_root(str(tmp_path), (H, W), n=1, seed=seed)
    img, disp, factor = samples[0]
    cfg = ref_shim._AttrDict(degree=1.0, random_crop=True, network_process_size=list(net))
    ds = RefDataset(mode, str(tmp_path), split, cfg, 1e-3, 80)
    random.seed(seed)
    np.random.seed(seed)
    want = ds[0]
    after = (random.random(), np.random.random())
    assert want["img_file_basename"] == "cene_Image0_00000"
    if mode != "train":
        assert torch.equal(want["image_hr"], torch.from_numpy(R.to_unit_f32(img).transpose(2, 0, 1)))
        assert torch.equal(want["depth_gt"], torch.from_numpy((np.float32(factor) / disp)[None]))
        return
    random.seed(seed)
    np.random.seed(seed)
    d = R.draw(1.0, (H, W), crop)
    got = R.host_sample(img, disp, factor, d, crop, net)
    assert after == (random.random(), np.random.random()), "the generators are left in the reference's state"
    m = R.rotate_matrix(d["angle"], W, H)
    depth = R.rotate_plane_nearest((np.float32(factor) / disp).astype(np.float32), R.fix16(m), d["flip"])
    assert torch.equal(want["depth_gt"], torch.from_numpy(depth[None])) and torch.equal(want["depth_gt"], got["depth_gt"])
    assert torch.equal(want["crop_depths"], got["crop_depths"]) and torch.equal(want["bboxs"], got["bboxs"])
    assert want["bboxs"].tolist() == [d["w0"], d["h0"], d["w0"] + crop[1], d["h0"] + crop[0]]
    assert want["image_hr"].tolist() == [H, W]
    unit = R.to_unit_f32(R.rotate_image_bilinear(img, m, d["flip"]))
    if d["colour"]:
        ref64 = torch.from_numpy(R.colour_f64(unit, d)[0].transpose(2, 0, 1))
        assert ((got["image"].double() - ref64).abs() <= POW_BAR * ref64.abs() + 1e-45).all()
        # the reference's resizes ran on ITS image: weights are non-negative and sum to one, so twice the bar carries over, plus six roundings of each resize
        for k in ("image_lr", "crops_image_hr"):
            assert float((want[k] - got[k]).abs().max()) <= 2 * POW_BAR + 12 * 2.0 ** -24
    else:
        assert torch.equal(got["image"], torch.from_numpy(unit.transpose(2, 0, 1)))
        assert torch.equal(want["image_lr"], got["image_lr"]) and torch.equal(want["crops_image_hr"], got["crops_image_hr"])
