"""numpy stand-in for the ground-truth entry point of hip_ops (same arguments and buffers), for depth_boundaries, and -- by reusing
tests/png_decode_fake_ops.py -- for the PNG-decode ops, so that groundtruth.read_depth_gt / read_pfm / read_npy and
datasets.ImageDataset run without a GPU.  gt_convert is written from the table of include/pf_hip.h on the PAYLOAD (bytes, kind, flags),
not from the loaders of tests/gt_ref.py: the two meet only in the tests."""
import numpy as np
import torch

from tests import eval_side_ref as E
from tests.png_decode_fake_ops import FakePngDecodeOps

F32 = np.float32


def _finite_or_zero(a):
    return np.where(np.isfinite(a), a, F32(0)).astype(F32)


class FakeGtOps(FakePngDecodeOps):
    def gt_convert(self, src, kind, mode, H, W, a, b, depth, edge_src=None, swap=False, flip=False):
        self.calls.append(("gt_convert", kind, mode, (H, W), bool(swap), bool(flip)))
        assert kind in ("f2", "f4", "f8", "u1", "u2") and mode in ("u4k", "mid", "eth3d", "gta", "cityscapes", "raw")
        floats = kind[0] == "f"
        assert {"u4k": floats, "raw": floats, "mid": kind == "f4", "eth3d": kind == "f4" and not swap,
                "gta": not floats and not swap, "cityscapes": not floats and not swap}[mode], (kind, mode, swap)
        raw = src.contiguous().view(torch.uint8).numpy().reshape(-1)
        assert raw.size == H * W * int(kind[1])
        x = raw.view(np.dtype(kind).newbyteorder(">" if swap else "<")).reshape(H, W)
        if flip:
            x = x[::-1]
        a, b = F32(a), F32(b)
        with np.errstate(all="ignore"):
            x = x.astype(F32)
            if mode == "u4k":
                d, e = a / x, x
            elif mode == "mid":
                d = np.where(x == np.inf, F32(0), (a / (x + b)) / F32(1000))
                e = np.where(x == np.inf, F32(0), x)
            elif mode == "eth3d":
                d = e = _finite_or_zero(x)
            elif mode == "gta":
                d = e = x / F32(256)
            elif mode == "cityscapes":
                d = e = _finite_or_zero(a / np.where(x > 0, (x - F32(1)) / F32(256), x))
            else:
                d = e = x
        depth.copy_(torch.from_numpy(np.ascontiguousarray(d, dtype=F32)))
        if edge_src is not None:
            edge_src.copy_(torch.from_numpy(np.ascontiguousarray(e, dtype=F32)))
        return depth

    def depth_boundaries(self, disp, th, dilation, out):
        self.calls.append(("depth_boundaries", float(th), int(dilation)))
        with np.errstate(all="ignore"):
            out.copy_(torch.from_numpy(E.get_boundaries(disp.numpy(), th, int(dilation))))
        return out

    def depth_metrics(self, gt, pred, edges, min_depth, max_depth, crop, out13, additional_mask=None):
        self.calls.append(("depth_metrics", float(min_depth), float(max_depth), tuple(crop), edges is not None))
        out13.zero_()
        return out13
