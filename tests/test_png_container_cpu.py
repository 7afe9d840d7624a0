"""CPU check of the host side of postprocess.encode_png with the numpy stand-in of tests/png_fake_ops.py in place of the kernels: the
band format (shared dynamic header, literals, end-of-block, sync flush), the Adler-32 combined from band partial sums and the PNG
container must give a file that PIL decodes to the input.  The kernels themselves are checked on the GPU (tests/test_png_gpu.py)."""
import io
import zlib

import numpy as np
import pytest
import torch
from PIL import Image

from patchfusion_amd import postprocess as post
from tests import png_ref as R
from tests.png_fake_ops import FakePngOps

CASES = [("u8c1", (9, 13)), ("u8c3", (17, 5)), ("u8c4", (3, 7)), ("u8c3_bgr", (10, 6)), ("u16", (11, 9)), ("u16", (1, 1))]


@pytest.mark.parametrize("fmt,shape", CASES, ids=[f"{f}-{s[0]}x{s[1]}" for f, s in CASES])
def test_container_round_trip_with_stand_in_kernels(fmt, shape):
    H, W = shape
    rng = np.random.default_rng(H * 31 + W)
    ch = {"u8c1": 1, "u8c3": 3, "u8c4": 4, "u8c3_bgr": 3, "u16": 1}[fmt]
    y, x, c = np.meshgrid(np.arange(H), np.arange(W), np.arange(ch), indexing="ij")
    a = (x * 37 + y * 301 + c * 5 + rng.integers(0, 3, (H, W, ch)))
    a = (a % 65536).astype(np.uint16)[..., 0] if fmt == "u16" else (a % 256).astype(np.uint8)
    a = np.ascontiguousarray(a if ch > 1 or fmt == "u16" else a[..., 0])
    bgr = fmt.endswith("bgr")
    png = post.encode_png(torch.from_numpy(a), bgr=bgr, ops=FakePngOps())
    got = np.asarray(Image.open(io.BytesIO(png)))
    want = a[..., ::-1] if bgr else a
    assert got.shape == want.shape and np.array_equal(got.astype(want.dtype), want)
    stream = zlib.decompress(R.idat_payload(png))
    assert len(stream) == H * (1 + W * ch * a.dtype.itemsize)
