"""Writes tests/golden/png_decode_cases.npz: PNG files written by PIL in every mode it can write, each with the array PIL decodes from
it, and two files from encode_png's CPU restatement (tests/png_fake_ops.py) with the arrays that went in.  Run from the repository root:
    python tools/make_golden_png_decode.py
Keys: <name>_png (the file's bytes) and <name>_expect (what decode_png must return)."""
import io
import os
import sys

import numpy as np
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from patchfusion_amd import postprocess  # noqa: E402
from tests import png_decode_ref as R  # noqa: E402
from tests.png_fake_ops import FakePngOps  # noqa: E402


def pil_bytes(im, **kw):
    b = io.BytesIO()
    im.save(b, "PNG", **kw)
    return b.getvalue()


def pil_expect(data):
    """what PIL decodes, in decode_png's layout: a palette goes to RGB, mode 1 to 0 / 255"""
    im = Image.open(io.BytesIO(data))
    if im.mode == "P":
        im = im.convert("RGB")
    a = np.asarray(im)
    if a.dtype == bool:
        a = a.astype(np.uint8) * 255
    return a.astype(np.uint16) if a.dtype.kind in "iu" and a.dtype.itemsize > 1 else a


def main():
    out = {}
    big = R.photo(150, 200, seed=2, noise=6.0)
    small = R.photo(37, 53, 4, seed=4)
    files = {
        "pil_rgb_150x200_l6": pil_bytes(Image.fromarray(big), compress_level=6),
        "pil_rgb_150x200_l1": pil_bytes(Image.fromarray(big), compress_level=1),
        "pil_l_37x53": pil_bytes(Image.fromarray(small[..., 0])),
        "pil_la_37x53": pil_bytes(Image.fromarray(small[..., :2], "LA")),
        "pil_rgba_37x53": pil_bytes(Image.fromarray(small, "RGBA")),
        "pil_1_37x53": pil_bytes(Image.fromarray(small[..., 0] > 128)),
        "pil_i16_37x53": pil_bytes(Image.fromarray(R.photo(37, 53, 1, seed=6, maximum=65535)[..., 0])),
        "pil_p8_37x53": pil_bytes(Image.fromarray(small[..., :3]).quantize(200)),
        "pil_p8_trns_37x53": pil_bytes(Image.fromarray(small[..., :3]).quantize(100), transparency=3),
    }
    for bits, colours in ((1, 2), (2, 4), (4, 16)):
        files[f"pil_p{bits}_37x53"] = pil_bytes(Image.fromarray(small[..., :3]).quantize(colours), bits=bits)
    for name, data in files.items():
        out[name + "_png"] = np.frombuffer(data, dtype=np.uint8)
        out[name + "_expect"] = pil_expect(data)
    ops = FakePngOps()
    depth = torch.from_numpy(R.photo(24, 40, 1, seed=8, maximum=65535)[..., 0].copy())
    colour = torch.from_numpy(R.photo(24, 40, 3, seed=9).copy())
    for name, x in (("encode_png_u16_24x40", depth), ("encode_png_rgb_24x40", colour)):
        out[name + "_png"] = np.frombuffer(postprocess.encode_png(x, ops=ops), dtype=np.uint8)
        out[name + "_expect"] = x.numpy()
    path = os.path.join(ROOT, "tests", "golden", "png_decode_cases.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;", len(files) + 2, "files")
    for name in sorted(k[:-4] for k in out if k.endswith("_png")):
        h = R.parse(out[name + "_png"].tobytes())
        print(f"  {name}: colour type {h['color_type']}, depth {h['depth']}, {out[name + '_png'].size} bytes -> {out[name + '_expect'].shape} "
              f"{out[name + '_expect'].dtype}")


if __name__ == "__main__":
    main()
