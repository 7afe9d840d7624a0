"""csrc/augment.hip on the GPU against the numpy restatement of tests/u4k_aug_ref.py (itself held to Pillow and to the reference by
tests/test_u4k_aug_ref_cpu.py), and one end-to-end UnrealStereo4kDataset.__getitem__('train').

Without the colour step every output is bit-equal: the rotation is Pillow's double arithmetic without contraction, / 255 one float32 division.
With it the chain holds a power, which numpy evaluates in float32 and the kernel in double: the kernel's error against the float64
restatement on the same operands must be within f64_image_ref.baseline_bar of numpy's own float32 result (at most twice the baseline, the
baseline floored at 4 * 2^-24), element-wise and normwise; no cap comes from the kernel's measured error.  Outputs are pre-filled with NaN
and every element must have been written.  37 x 53 and 64 x 96 are odd / not multiples of the four-pixel groups and take the scalar- and
the vector-store kernels; 2160 x 3840 is the only size at which the 16.16 sums and the double coordinates reach their working range."""
import random

import numpy as np
import pytest
import torch

from tests import f64_image_ref as I
from tests import u4k_aug_ref as R

pytestmark = pytest.mark.gpu

COLOUR = dict(colour=True, gamma=1.0731, brightness=0.9312, colours=np.array([0.9137, 1.0921, 1.0043]))
PLAIN = dict(colour=False)


@pytest.fixture(scope="module")
def ops():
    from patchfusion_amd.hip_ops import ops as hip
    return hip


def inputs(H, W, seed):
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    img[: H // 4, : W // 4] = 0                                           # 0 ** gamma, and black against the zero fill
    img[-(H // 4):, -(W // 4):] = 255                                     # the clip at 1
    return img, (rng.random((H, W), dtype=np.float32) * 180 + 2).astype(np.float32), (rng.random((H, W), dtype=np.float32) + 0.5).astype(np.float32)


def run_image(ops, img, m, flip, d):
    H, W, _ = img.shape
    out = torch.full((3, H, W), float("nan"), device="cuda")
    colour = (d["gamma"], d["brightness"], d["colours"]) if d["colour"] else None
    ops.aug_image_u8_to_f32(torch.from_numpy(img).cuda(), m, flip, colour, out)
    y = out.cpu()
    assert not torch.isnan(y).any(), "every element is written"
    return y


def check_image(y, img, m, flip, d, what):
    unit = R.to_unit_f32(R.rotate_image_bilinear(img, m, flip))
    if not d["colour"]:
        assert torch.equal(y, torch.from_numpy(unit.transpose(2, 0, 1))), what
        return
    ref, mag = (torch.from_numpy(np.ascontiguousarray(a.transpose(2, 0, 1))) for a in R.colour_f64(unit, d))
    e = I.errors(y, ref, mag)
    b = I.errors(torch.from_numpy(np.ascontiguousarray(R.colour_f32(unit, d).transpose(2, 0, 1))), ref, mag)
    print(f"{what}: kernel {e[0]:.3e} / {e[1]:.3e}, numpy float32 {b[0]:.3e} / {b[1]:.3e} (element-wise / normwise)")
    assert I.baseline_bar(e, b), (what, e, b)


def run_planes(ops, planes, fixed, flip):
    outs = [torch.full(p.shape, float("nan"), device="cuda") for p in planes]
    ops.aug_planes_nearest([torch.from_numpy(p).cuda() for p in planes], fixed, flip, outs)
    outs = [o.cpu() for o in outs]
    assert not any(torch.isnan(o).any() for o in outs), "every element is written"
    return outs


@pytest.mark.parametrize("H,W,degree", [(37, 53, 5.0), (64, 96, 5.0), (64, 96, 1.0)])
def test_kernels_equal_the_restatement(ops, H, W, degree):
    img, p0, p1 = inputs(H, W, H)
    for angle in (0.0, degree, -degree):
        m = R.rotate_matrix(angle, W, H)
        fixed = R.fix16(m)
        for flip in (False, True):
            want = [torch.from_numpy(R.rotate_plane_nearest(p, fixed, flip)) for p in (p0, p1)]
            got = run_planes(ops, [p0, p1], fixed, flip)
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), (angle, flip)
            assert torch.equal(run_planes(ops, [p1], fixed, flip)[0], want[1]), (angle, flip)
            for d in (PLAIN, COLOUR):
                check_image(run_image(ops, img, m, flip, d), img, m, flip, d, f"{H}x{W} angle {angle} flip {flip} colour {d['colour']}")


def test_rotation_at_full_size(ops):
    H, W = 2160, 3840
    img, p0, _ = inputs(H, W, 3)
    angle = -0.8731
    m = R.rotate_matrix(angle, W, H)
    assert torch.equal(run_planes(ops, [p0], R.fix16(m), False)[0], torch.from_numpy(R.rotate_plane_nearest(p0, R.fix16(m))))
    check_image(run_image(ops, img, m, False, PLAIN), img, m, False, PLAIN, "2160x3840")


def test_entry_points_refuse_what_the_header_says(ops):
    img = torch.zeros((8, 8, 3), dtype=torch.uint8, device="cuda")
    out = torch.empty((3, 8, 8), device="cuda")
    m = R.rotate_matrix(1.0, 8, 8)
    from patchfusion_amd._lib import PfError
    with pytest.raises(PfError):
        ops.aug_image_u8_to_f32(img, m[:5] + [float("nan")], False, None, out)
    plane = torch.zeros((8, 8), device="cuda")
    with pytest.raises(PfError):
        ops.aug_planes_nearest([plane], R.fix16(m), False, [plane])                  # in place


class Recording:
    """the ops with the augmented image kept: __getitem__ does not return it"""

    def __init__(self, ops):
        self._ops, self.image = ops, None

    def __getattr__(self, name):
        return getattr(self._ops, name)

    def aug_image_u8_to_f32(self, *a):
        self.image = self._ops.aug_image_u8_to_f32(*a)
        return self.image


@pytest.mark.parametrize("seed", [0, 4])                                   # colour and flip on; both off
def test_train_sample_end_to_end(ops, tmp_path, seed):
    from patchfusion_amd.datasets import UnrealStereo4kDataset
    IMAGE, PATCH, NET = (448, 616), (224, 308), (112, 154)
    split, samples = R.write_root(str(tmp_path), IMAGE, n=1, seed=seed)
    img, disp, factor = samples[0]
    rec = Recording(ops)
    ds = UnrealStereo4kDataset("train", str(tmp_path), split, dict(degree=1.0, random_crop=True, network_process_size=list(NET)), 1e-3, 80,
                               patch_raw_shape=PATCH, resize_mode="depth-anything", device="cuda", ops=rec, image_shape=IMAGE)
    random.seed(seed)
    np.random.seed(seed)
    s = ds[0]
    after = (random.random(), np.random.random())
    random.seed(seed)
    np.random.seed(seed)
    d = R.draw(1.0, IMAGE, PATCH)
    assert after == (random.random(), np.random.random()), "the generators are left in the reference's state"
    assert all(v.is_cuda for k, v in s.items() if k != "img_file_basename")
    m = R.rotate_matrix(d["angle"], IMAGE[1], IMAGE[0])
    depth = R.rotate_plane_nearest((np.float32(factor) / disp).astype(np.float32), R.fix16(m), d["flip"])
    h0, w0 = d["h0"], d["w0"]
    box = [w0, h0, w0 + PATCH[1], h0 + PATCH[0]]
    assert torch.equal(s["depth_gt"].cpu(), torch.from_numpy(depth[None]))
    assert torch.equal(s["crop_depths"].cpu(), torch.from_numpy(depth[None, h0:h0 + PATCH[0], w0:w0 + PATCH[1]].copy()))
    assert s["bboxs"].tolist() == box and s["image_hr"].tolist() == list(IMAGE)
    image = rec.image.cpu()
    check_image(image, img, m, d["flip"], d, f"train sample, seed {seed}")
    for c in range(3):
        ref, mag = I.bilinear_plane_ref(image[c], *NET)
        ok, worst = I.counted_bar(s["image_lr"][c], ref, mag, 6)
        assert ok, ("image_lr", c, worst)
    ref, mag = I.crop_resize_ref(image, torch.tensor([box]), *NET)
    ok, worst = I.counted_bar(s["crops_image_hr"][None], ref, mag, 6)
    assert ok, ("crops_image_hr", worst)
