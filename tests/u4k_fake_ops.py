"""torch stand-ins for the two augmentation entry points of hip_ops (same arguments and buffers), written from the prototypes' description
in include/pf_hip.h, not from tests/u4k_aug_ref.py: the two meet only in the tests.  On top of tests/gt_fake_ops.py (ground truth, edges)
and with the real torch resizes of tests/fake_ops.py, so that datasets.UnrealStereo4kDataset runs in both modes without a GPU."""
import numpy as np
import torch

from tests.fake_ops import FakeOps
from tests.gt_fake_ops import FakeGtOps

F64 = torch.float64


class FakeU4kOps(FakeGtOps):
    u8_bicubic_to_f32 = staticmethod(FakeOps.u8_bicubic_to_f32)
    resize_bilinear_f32 = staticmethod(FakeOps.resize_bilinear_f32)
    crop_resize = staticmethod(FakeOps.crop_resize)

    def aug_image_u8_to_f32(self, img_u8, matrix, flip, colour, out):
        self.calls.append(("aug_image", tuple(img_u8.shape), bool(flip), colour is not None))
        H, W, _ = img_u8.shape
        assert img_u8.dtype == torch.uint8 and tuple(out.shape) == (3, H, W) and out.dtype == torch.float32
        m = [float(v) for v in matrix]
        x = torch.arange(W, dtype=F64)
        xc = ((W - 1 - x) if flip else x)[None, :] + 0.5
        yc = torch.arange(H, dtype=F64)[:, None] + 0.5
        xs = m[0] * xc + m[1] * yc + m[2]
        ys = m[3] * xc + m[4] * yc + m[5]
        outside = (xs < 0) | (xs >= W) | (ys < 0) | (ys >= H)
        xin, yin = xs - 0.5, ys - 0.5
        x0, y0 = torch.floor(xin), torch.floor(yin)
        dx, dy = (xin - x0)[..., None], (yin - y0)[..., None]
        x0, y0 = x0.long(), y0.long()
        xa, xb = x0.clamp(0, W - 1), (x0 + 1).clamp(0, W - 1)
        ya, yb = y0.clamp(0, H - 1), y0 + 1
        below = ((yb >= 0) & (yb < H))[..., None]
        yb = yb.clamp(0, H - 1)
        src = img_u8.to(F64)
        v1 = src[ya, xa] + (src[ya, xb] - src[ya, xa]) * dx
        v2 = torch.where(below, src[yb, xa] + (src[yb, xb] - src[yb, xa]) * dx, v1)
        v = torch.where(outside[..., None], torch.zeros((), dtype=F64), v1 + (v2 - v1) * dy)
        v = v.to(torch.uint8).float().flip(-1) / torch.tensor(255.0, dtype=torch.float32)                  # truncation; B, G, R -> R, G, B
        if colour is not None:
            gamma, brightness, colours = colour
            v = torch.pow(v.double(), float(np.float32(gamma))).float()
            v = v * torch.tensor(float(np.float32(brightness)), dtype=torch.float32)
            v = (v.double() * torch.tensor([float(c) for c in colours], dtype=F64)).float().clamp(0, 1)
        out.copy_(v.permute(2, 0, 1))
        return out

    def aug_planes_nearest(self, srcs, fixed, flip, outs):
        self.calls.append(("aug_planes", len(srcs), bool(flip)))
        H, W = srcs[0].shape
        a = [int(v) for v in fixed]
        x = torch.arange(W, dtype=torch.int64)
        xp = ((W - 1 - x) if flip else x)[None, :]
        y = torch.arange(H, dtype=torch.int64)[:, None]
        sx = (a[2] + xp * a[0] + y * a[1]) >> 16
        sy = (a[5] + xp * a[3] + y * a[4]) >> 16
        inside = (sx >= 0) & (sx < W) & (sy >= 0) & (sy < H)
        for s, o in zip(srcs, outs):
            assert s.dtype == o.dtype == torch.float32 and tuple(o.shape) == (H, W)
            o.copy_(torch.where(inside, s[sy.clamp(0, H - 1), sx.clamp(0, W - 1)], torch.zeros((), dtype=torch.float32)))
        return outs
