"""numpy stand-in for the JPEG entry points of hip_ops (same arguments and buffers), built on tests/jpeg_ref.py, so that the host side of
preprocess.decode_jpeg and ImagePreprocessor.read can be checked without a GPU (the pattern of tests/png_fake_ops.py)."""
import numpy as np
import torch

from tests import jpeg_ref as R


class FakeJpegOps:
    def __init__(self, data):
        self.data, self.calls = data, []

    def jpeg_workspace(self, header, nlanes):
        return 16 + 28 * nlanes, 64

    def jpeg_decode_entropy(self, header, scan, lanes, segx, longest, tables, max_sync_rounds, workspace, coef):
        S = int(lanes[0, 1] - lanes[0, 0]) if lanes.shape[0] > 1 else 1 << 20
        _, rounds, _ = R.sync_model(self.data, S)
        self.calls.append(("entropy", S, int(max_sync_rounds)))
        if rounds > max_sync_rounds:
            return 64, max_sync_rounds
        coef.copy_(torch.from_numpy(R.decode_entropy(self.data)))
        return 0, rounds

    def jpeg_reconstruct(self, header, coef, orientation, workspace, rgb):
        self.calls.append(("reconstruct", int(orientation)))
        rgb.copy_(torch.from_numpy(R.reconstruct(R.parse(self.data), coef.numpy(), orientation)))
        return rgb

    # the two resizes ImagePreprocessor.__call__ runs: only recorded
    def u8_bicubic_to_f32(self, img, out, reverse_channels=False):
        self.calls.append(("bicubic", tuple(img.shape)))
        out.zero_()

    def resize_bilinear_f32(self, src, dst):
        dst.zero_()
