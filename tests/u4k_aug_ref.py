"""numpy restatement of the training-side augmentations of the reference's UnrealStereo4kDataset (estimator/datasets/u4k_dataset.py:110-178,
transformers/augmentations.py), written from Pillow's C sources and numpy's casting rules, not from the kernels of csrc/augment.hip:

  * the affine matrix of Image.rotate (rotate_matrix) and its 16.16 form (fix16),
  * Image.rotate(angle, resample=BILINEAR) on an RGB image, in float64 exactly as Pillow's bilinear_filter32RGB (rotate_image_bilinear),
  * Image.rotate(angle, resample=NEAREST) on a mode-'F' plane, Pillow's fixed-point affine path (rotate_plane_nearest),
  * `image.astype(float32)[:, :, ::-1] / 255.0` and aug_color, once in float64 (the reference of the graded comparison: colour_f64) and once
    as numpy does it in float32 (the baseline of that comparison and the bit-exact restatement of everything but `**`: colour_f32),
  * the draws of one __getitem__ in the reference's order (draw),
  * host_sample: the whole train sample on the host with Pillow and numpy, operation by operation as the reference (the host side of
    tools/u4k_dataset_time.py).
checked on the CPU by tests/test_u4k_aug_ref_cpu.py (against Pillow, against the reference's own functions, against a committed fixture)."""
import math
import random

import numpy as np

F32 = np.float32


# ---------------- the draws ----------------
def draw(degree, image_shape, crop_shape):
    """every random number of one train __getitem__, from Python's `random` and np.random in the reference's order: aug_rotate, aug_color,
    aug_flip, random_crop.  -> dict(angle, colour (bool), gamma, brightness, colours float64 [3], flip (bool), h0, w0)"""
    d = dict(angle=(random.random() - 0.5) * 2 * degree, gamma=1.0, brightness=1.0, colours=np.ones(3))
    d["colour"] = random.random() > 0.5
    if d["colour"]:
        d["gamma"] = random.uniform(0.9, 1.1)
        d["brightness"] = random.uniform(0.9, 1.1)
        d["colours"] = np.random.uniform(0.9, 1.1, size=3)
    d["flip"] = random.random() > 0.5
    d["h0"] = random.randint(0, image_shape[0] - crop_shape[0])
    d["w0"] = random.randint(0, image_shape[1] - crop_shape[1])
    return d


# ---------------- the matrix ----------------
def rotate_matrix(angle, W, H):
    """Image.rotate's matrix (PIL/Image.py), in Python floats: output pixel centre -> source position"""
    angle = angle % 360.0
    a = -math.radians(angle)
    m = [round(math.cos(a), 15), round(math.sin(a), 15), 0.0, round(-math.sin(a), 15), round(math.cos(a), 15), 0.0]
    cx, cy = W / 2.0, H / 2.0

    def transform(x, y):
        return m[0] * x + m[1] * y + m[2], m[3] * x + m[4] * y + m[5]
    m[2], m[5] = transform(-cx, -cy)
    m[2] += cx
    m[5] += cy
    return m


def fix16(m):
    """the six 16.16 integers of ImagingTransformAffine's nearest path (Geometry.c): FIX(v) = floor(v * 65536 + 0.5)"""
    fix = lambda v: int(math.floor(v * 65536.0 + 0.5))                  # noqa: E731
    return [fix(m[0]), fix(m[1]), fix(m[2] + m[0] * 0.5 + m[1] * 0.5), fix(m[3]), fix(m[4]), fix(m[5] + m[3] * 0.5 + m[4] * 0.5)]


# ---------------- the rotations ----------------
def rotate_image_bilinear(img, m, flip=False, rows=256):
    """img uint8 [H,W,C] -> uint8 [H,W,C]: output (y, x) is the rotated image at (flip ? W-1-x : x, y).  Every product and sum is its own
    float64 operation (numpy never fuses), the result is truncated."""
    H, W, C = img.shape
    out = np.empty_like(img)
    xp = np.arange(W, dtype=np.float64)
    if flip:
        xp = xp[::-1]
    xc = (xp + 0.5)[None, :]
    for r0 in range(0, H, rows):
        yc = (np.arange(r0, min(r0 + rows, H), dtype=np.float64) + 0.5)[:, None]
        xs = m[0] * xc + m[1] * yc + m[2]
        ys = m[3] * xc + m[4] * yc + m[5]
        outside = (xs < 0) | (xs >= W) | (ys < 0) | (ys >= H)
        xin, yin = xs - 0.5, ys - 0.5
        fx, fy = np.floor(xin), np.floor(yin)
        dx, dy = (xin - fx)[..., None], (yin - fy)[..., None]
        x0, y0 = fx.astype(np.int64), fy.astype(np.int64)
        xa, xb = np.clip(x0, 0, W - 1), np.clip(x0 + 1, 0, W - 1)
        ya = np.clip(y0, 0, H - 1)
        below = ((y0 + 1 >= 0) & (y0 + 1 < H))[..., None]
        yb = np.clip(y0 + 1, 0, H - 1)
        p, q = img[ya, xa].astype(np.float64), img[ya, xb].astype(np.float64)
        v1 = p + (q - p) * dx
        p, q = img[yb, xa].astype(np.float64), img[yb, xb].astype(np.float64)
        v2 = np.where(below, p + (q - p) * dx, v1)
        v = v1 + (v2 - v1) * dy
        out[r0:r0 + yc.shape[0]] = np.where(outside[..., None], 0.0, v).astype(np.uint8)      # values in [0, 255]: truncation
    return out


def rotate_plane_nearest(plane, a, flip=False):
    """plane float32 [H,W] -> float32 [H,W] with the six integers of fix16; 0 outside"""
    H, W = plane.shape
    xp = np.arange(W, dtype=np.int64)
    if flip:
        xp = xp[::-1]
    y = np.arange(H, dtype=np.int64)[:, None]
    sx = (a[2] + xp[None, :] * a[0] + y * a[1]) >> 16
    sy = (a[5] + xp[None, :] * a[3] + y * a[4]) >> 16
    assert max(abs(a[2]) + W * abs(a[0]) + H * abs(a[1]), abs(a[5]) + W * abs(a[3]) + H * abs(a[4])) < 2 ** 31     # Pillow's int
    inside = (sx >= 0) & (sx < W) & (sy >= 0) & (sy < H)
    return np.where(inside, plane[np.clip(sy, 0, H - 1), np.clip(sx, 0, W - 1)], F32(0)).astype(F32)


# ---------------- the colour path ----------------
def to_unit_f32(img_bgr):
    """u4k_dataset.py:126-129: uint8 [H,W,3] in file order -> float32 [H,W,3] RGB in [0, 1], one float32 division"""
    return img_bgr.astype(F32)[:, :, ::-1].copy() / 255.0


def colour_f32(image, d):
    """aug_color's arithmetic on a float32 [H,W,3] image with the draws d, as numpy does it: float32 `**` and `*` by the Python floats,
    the product with the float64 colours formed in double and stored to float32, the clip"""
    if not d["colour"]:
        return image
    aug = image ** d["gamma"]
    aug = aug * d["brightness"]
    assert aug.dtype == F32
    aug *= np.broadcast_to(np.asarray(d["colours"], dtype=np.float64), image.shape)
    return np.clip(aug, 0, 1)


def colour_f64(image, d):
    """the same on the same operands (the float32 image, float32(gamma), float32(brightness), the float64 colours) in float64 throughout:
    -> (ref, mag) float64, mag = |ref| (a chain of products)"""
    v = image.astype(np.float64)
    if d["colour"]:
        v = np.clip(v ** float(F32(d["gamma"])) * float(F32(d["brightness"])) * np.asarray(d["colours"], dtype=np.float64), 0, 1)
    return v, np.abs(v)


def image_ref(img_bgr, d, flip=None):
    """uint8 [H,W,3] in file order + draws -> (rotated uint8 [H,W,3] RGB, flipped; the float32 unit image before the colour step [H,W,3])"""
    H, W, _ = img_bgr.shape
    rot = rotate_image_bilinear(img_bgr, rotate_matrix(d["angle"], W, H), d["flip"] if flip is None else flip)
    return rot[:, :, ::-1], to_unit_f32(rot)


# ---------------- the whole sample on the host ----------------
def host_sample(img_bgr, disp, depth_factor, d, crop_shape, process_shape, stages=None):
    """one train sample from the decoded inputs with Pillow, numpy and torch on the CPU, the reference's operations in its order (the
    draws d already made) -> torch tensors.  stages: a dict that receives the seconds of 'ground_truth', 'planes', 'image', 'resizes'."""
    import time

    from PIL import Image
    t = [time.perf_counter()]

    def tick(key):
        if stages is not None:
            now = time.perf_counter()
            stages[key] = stages.get(key, 0.0) + now - t[0]
            t[0] = now
    disp = disp.astype(F32)
    depth = depth_factor / disp
    tick("ground_truth")
    image = np.asarray(Image.fromarray(img_bgr).rotate(d["angle"], resample=Image.BILINEAR)).copy()
    tick("image")
    depth = np.asarray(Image.fromarray(depth).rotate(d["angle"], resample=Image.NEAREST)).copy()
    disp = np.asarray(Image.fromarray(disp).rotate(d["angle"], resample=Image.NEAREST)).copy()
    tick("planes")
    image = colour_f32(to_unit_f32(image), d)
    if d["flip"]:
        image = image[:, ::-1].copy()
    tick("image")
    if d["flip"]:
        depth, disp = depth[:, ::-1].copy(), disp[:, ::-1].copy()
    tick("planes")
    import torch
    import torch.nn.functional as F
    chw = torch.from_numpy(image.transpose(2, 0, 1))                     # to_tensor: a strided view, as in the reference
    h, w = crop_shape
    h0, w0 = d["h0"], d["w0"]

    def resize(t):                                                        # midas.Resize on a tensor
        return F.interpolate(t.unsqueeze(0), tuple(process_shape), mode="bilinear", align_corners=True).squeeze(0)
    ret = dict(image=chw, image_lr=resize(chw), depth_gt=torch.from_numpy(depth[None]),
               crops_image_hr=resize(chw[:, h0:h0 + h, w0:w0 + w].clone()), crop_depths=torch.from_numpy(depth[None, h0:h0 + h, w0:w0 + w].copy()),
               bboxs=torch.tensor([w0, h0, w0 + w, h0 + h]))
    tick("resizes")
    return ret


# ---------------- a synthetic data root ----------------
def write_root(root, image_shape, n=1, seed=0):
    """n samples in the dataset's layout under `root` (scene/Image0/*.raw, Disp0/*.npy, Extrinsics0|1/*.txt) and a split file with the
    four columns of the reference's lists -> (split path, [(image uint8 [H,W,3] in file order, disparity float32 [H,W], depth factor)])"""
    import os
    H, W = image_shape
    rng = np.random.default_rng(seed)
    lines, samples = [], []
    for i in range(n):
        name = f"{i:05d}"
        for sub in ("Image0", "Disp0", "Extrinsics0", "Extrinsics1"):
            os.makedirs(os.path.join(root, "scene", sub), exist_ok=True)
        img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        disp = (rng.random((H, W), dtype=F32) * F32(180) + F32(2)).astype(F32)
        focal, tl, tr = 1109.25 + i, -0.05, 0.05 + 0.001 * i             # depths of 0.6 .. 56: inside the evaluated range
        img.tofile(os.path.join(root, "scene", "Image0", name + ".raw"))
        np.save(os.path.join(root, "scene", "Disp0", name + ".npy"), disp)
        for sub, t in (("Extrinsics0", tl), ("Extrinsics1", tr)):
            with open(os.path.join(root, "scene", sub, name + ".txt"), "w") as f:
                f.write(f"{focal!r} 0.0 {W / 2!r}\n1.0 0.0 0.0 {t!r}\n")
        lines.append(f"scene/Image0/{name}.png scene/Image1/{name}.png scene/Disp0/{name}.npy scene/Disp1/{name}.npy")
        samples.append((img, disp, abs(tl - tr) * focal))
    split = os.path.join(root, "split.txt")
    with open(split, "w") as f:
        f.write("\n".join(lines[::-1]) + "\n")                               # out of order: load_data_list sorts
    return split, samples
