"""Writes tests/golden/jpeg_prog_cases.npz: progressive JPEG files and the uint8 RGB arrays PIL (libjpeg-turbo) decodes them to.
jpeg_<name> = the file's bytes, rgb_<name> = the expected [H,W,3] array (absent for the files that must be refused).  The PIL-made files
carry libjpeg's default ten-scan script; the w_* files are made by the writer of tests/jpeg_prog_ref.py from the coefficients of the
100x75 file, with the scripts PIL cannot choose.  The GPU tests read only this file.  Run from the repository root:
python tools/make_golden_jpeg_prog.py"""
import os
import sys

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import jpeg_prog_ref as G  # noqa: E402
from tests import jpeg_ref as R  # noqa: E402

# scan scripts: (components, Ss, Se, Ah, Al)
EXAMPLE_2 = [((0, 1, 2), 0, 0, 0, 0), ((0,), 1, 8, 0, 2), ((0,), 9, 63, 0, 2), ((0,), 1, 63, 2, 1), ((0,), 1, 63, 1, 0), ((1,), 1, 63, 0, 0),
             ((2,), 1, 63, 0, 0)]
EXAMPLE_3 = [((0, 1, 2), 0, 0, 0, 0), ((0,), 1, 2, 0, 1), ((0,), 3, 63, 0, 1), ((0,), 1, 63, 1, 0), ((1,), 1, 2, 0, 0), ((1,), 3, 63, 0, 0),
             ((2,), 1, 2, 0, 0), ((2,), 3, 63, 0, 0)]
NONINTERLEAVED_DC = [((0,), 0, 0, 0, 1), ((1,), 0, 0, 0, 0), ((2,), 0, 0, 0, 1), ((0,), 1, 63, 0, 0), ((2,), 0, 0, 1, 0), ((0,), 0, 0, 1, 0),
                     ((1,), 1, 63, 0, 0), ((2,), 1, 63, 0, 0)]
LONG_RUN = [((0, 1, 2), 0, 0, 0, 0), ((0,), 1, 63, 0, 1), ((1,), 1, 63, 0, 0), ((2,), 1, 63, 0, 0), ((0,), 1, 63, 1, 0)]
INCOMPLETE = EXAMPLE_2[:4] + EXAMPLE_2[5:]                     # luma stays at bit 1
NO_FIRST = [EXAMPLE_3[0], EXAMPLE_3[2], EXAMPLE_3[3]]          # the refinement of 1-63 meets 1-2 that were never sent
TWO_COMPONENT_AC = [((0, 1, 2), 0, 0, 0, 0), ((1, 2), 1, 63, 0, 0)]


def main():
    out = {}

    def add(name, data, transpose=False, expect=True):
        out["jpeg_" + name] = np.frombuffer(data, dtype=np.uint8)
        if expect:
            out["rgb_" + name] = R.pil_decode(data, transpose)

    enc = lambda a, **kw: R.pil_encode(a, progressive=True, **kw)      # noqa: E731
    base = enc(R.image("smooth", 75, 100, 2001), quality=75, subsampling="4:2:0")
    add("100x75_smooth_420_q75", base)                                  # luma: 13 x 10 real blocks in a 14 x 10 padded grid
    add("37x53_noise_444_q95", enc(R.image("noise", 37, 53, 2002), quality=95, subsampling="4:4:4"))
    add("64x48_smooth_422_q50", enc(R.image("smooth", 48, 64, 2003), quality=50, subsampling="4:2:2"))
    add("17x19_grey", enc(R.image("smooth", 17, 19, 2004, grey=True), quality=90))
    add("1x1", enc(R.image("noise", 1, 1, 2005), quality=90, subsampling="4:2:0"))
    add("64x64_constant", enc(np.full((64, 64, 3), (200, 90, 30), dtype=np.uint8), quality=90, subsampling="4:2:0"))
    add("256x256_smooth_q30", enc(R.image("smooth", 256, 256, 2006), quality=30, subsampling="4:2:0"))
    add("256x256_noise_q100", enc(R.image("noise", 256, 256, 2007), quality=100, subsampling="4:2:0"))
    add("100x75_smooth_420_rst", enc(R.image("smooth", 75, 100, 2001), quality=75, subsampling="4:2:0", restart_blocks=3))
    exif = Image.Exif()
    exif[0x0112] = 6
    add("orient6_17x19", enc(R.image("smooth", 17, 19, 2008), quality=90, subsampling="4:2:0", exif=exif.tobytes()), transpose=True)

    parsed = G.parse(base)
    h, coef = parsed[0], G.decode_entropy(base, parsed)
    add("w_example2_script", G.write(h, coef, EXAMPLE_2))
    add("w_example3_script", G.write(h, coef, EXAMPLE_3))
    add("w_noninterleaved_dc", G.write(h, coef, NONINTERLEAVED_DC))
    sparse = coef.copy()
    keep = np.zeros(h.nblocks, dtype=bool)
    keep[::97] = True                                                   # one block in 97 keeps its AC coefficients: EOB runs of ~60 luma blocks
    sparse[~keep, 1:] = 0
    add("w_long_eob_run", G.write(h, sparse, LONG_RUN))
    add("refuse_incomplete", G.write(h, coef, INCOMPLETE), expect=False)
    add("refuse_no_first", G.write(h, coef, NO_FIRST), expect=False)
    add("refuse_two_component_ac", G.write(h, coef, TWO_COMPONENT_AC), expect=False)
    path = os.path.join(ROOT, "tests", "golden", "jpeg_prog_cases.npz")
    np.savez_compressed(path, **out)
    print(path, len(out), "arrays", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
