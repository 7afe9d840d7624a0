"""Writes tests/golden/jpeg_cases.npz: seeded JPEG files (encoded with PIL) and the uint8 RGB arrays PIL (libjpeg-turbo: islow inverse DCT,
fancy upsampling) decodes them to.  jpeg_<name> = the file's bytes, rgb_<name> = the expected [H,W,3] array (absent for the two files that
must be refused).  The GPU tests read only this file.  Run from the repository root: python tools/make_golden_jpeg.py"""
import io
import os
import sys

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import jpeg_ref as R  # noqa: E402

SIZES = [(1, 1), (8, 8), (16, 16), (15, 16), (17, 19), (33, 7), (37, 53), (64, 48)]
SUBS = ["4:4:4", "4:2:2", "4:2:0", "grey"]
SETTINGS = {"q30": dict(quality=30), "q90": dict(quality=90), "q100": dict(quality=100), "opt": dict(quality=90, optimize=True),
            "rst": dict(quality=90, restart_blocks=1)}


def main():
    out = {}

    def add(name, data, transpose=False, expect=True):
        out["jpeg_" + name] = np.frombuffer(data, dtype=np.uint8)
        if expect:
            out["rgb_" + name] = R.pil_decode(data, transpose)

    seed = 0
    for si, (H, W) in enumerate(SIZES):
        for bi, sub in enumerate(SUBS):
            for ki, kind in enumerate(("noise", "smooth")):
                # every setting on 17x19 and on the 4:4:4 and 4:2:0 noise of 37x53, one setting in turn elsewhere
                for i, (sname, kw) in enumerate(SETTINGS.items()):
                    seed += 1
                    every = (H, W) == (17, 19) or ((H, W) == (37, 53) and kind == "noise" and sub in ("4:4:4", "4:2:0"))
                    if not every and i != (si + bi + ki) % 5:
                        continue
                    a = R.image(kind, H, W, seed, grey=sub == "grey")
                    add(f"{H}x{W}_{kind}_{sub.replace(':', '')}_{sname}", R.pil_encode(a, subsampling=None if sub == "grey" else sub, **kw))
    add("256x256_noise_q100", R.pil_encode(R.image("noise", 256, 256, 1001), quality=100, subsampling="4:2:0"))
    add("256x256_smooth_q30", R.pil_encode(R.image("smooth", 256, 256, 1002), quality=30, subsampling="4:2:0"))
    add("64x48_smooth_rstrow", R.pil_encode(R.image("smooth", 48, 64, 1003), quality=90, subsampling="4:2:0", restart_rows=1))
    for o in range(1, 9):
        exif = Image.Exif()
        exif[0x0112] = o
        add(f"orient{o}_17x19", R.pil_encode(R.image("smooth", 17, 19, 1010 + o), quality=90, subsampling="4:2:0", exif=exif.tobytes()), transpose=True)
    add("refuse_progressive", R.pil_encode(R.image("smooth", 16, 16, 1020), progressive=True), expect=False)
    buf = io.BytesIO()
    Image.fromarray(R.image("smooth", 16, 16, 1021)).convert("CMYK").save(buf, "JPEG")
    add("refuse_cmyk", buf.getvalue(), expect=False)
    path = os.path.join(ROOT, "tests", "golden", "jpeg_cases.npz")
    np.savez_compressed(path, **out)
    print(path, len(out), "arrays", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
