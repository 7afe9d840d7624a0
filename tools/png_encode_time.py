"""Times postprocess.encode_png on the 1568x2072 fixture of DESIGN 9b: strategies 'huffman', 'rle' and 'auto' for the 16-bit and the
colour image, interleaved in one process after warm-up, seven repetitions, median (min-max), with the file sizes.  With
--parent-lib PATH (a libpf_hip.so built from the parent commit) the literal-only encode of that library is timed in the same
interleaved loop as `huffman_parent`: the check that the default path did not move.  Numbers are of one box; --out writes the JSON.

    python tools/png_encode_time.py --parent-lib /path/to/parent/libpf_hip.so --out profiles/png_rle_encode_time.json
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from patchfusion_amd import postprocess as post  # noqa: E402
from patchfusion_amd.hip_ops import HipOps, _p, _stream  # noqa: E402


class LibPngOps:
    """the four literal-only PNG entry points of another build of the library, behind the interface encode_png expects"""
    PNG_BAND_ROWS = HipOps.PNG_BAND_ROWS
    png_format = staticmethod(HipOps.png_format)

    def __init__(self, path):
        self.lib = C.CDLL(path)

    def png_workspace(self, image, bgr=False):
        H, W, ch, bits, _ = self.png_format(image, bgr)
        ws, ob, nb = C.c_long(), C.c_long(), C.c_int()
        assert self.lib.pf_png_workspace_bytes(H, W, ch, bits, C.byref(ws), C.byref(ob), C.byref(nb)) == 0
        return ws.value, ob.value, nb.value

    def png_filter_histogram(self, image, workspace, hist, bgr=False):
        H, W, ch, bits, bgr = self.png_format(image, bgr)
        assert self.lib.pf_png_filter_histogram(_p(image), H, W, ch, bits, bgr, _p(workspace), _p(hist), _stream()) == 0

    def png_build_table(self, hist):
        h = np.ascontiguousarray(hist, dtype=np.uint32)
        table = np.zeros(HipOps.PNG_TABLE_WORDS, dtype=np.uint32)
        u32p = C.POINTER(C.c_uint32)
        assert self.lib.pf_png_build_table(h.ctypes.data_as(u32p), table.ctypes.data_as(u32p)) == 0
        return table

    def png_encode(self, image, table, workspace, out, meta, bgr=False):
        H, W, ch, bits, bgr = self.png_format(image, bgr)
        assert self.lib.pf_png_encode(_p(image), H, W, ch, bits, bgr, _p(table), _p(workspace), _p(out), _p(meta),
                                      _stream()) == 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib")
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    H, W = 1568, 2072
    y, x = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    d = 5 + 3 * np.sin(x / 300) * np.cos(y / 200) + 0.002 * np.random.default_rng(0).standard_normal((H, W))
    dev = torch.from_numpy(d.astype(np.float32)).cuda()
    images = {"u16": (post.depth_to_uint16(dev), False), "rgb": (post.colorize(dev, cmap="magma_r", layout="bgr"), True)}
    arms = {}
    for key, (img, bgr) in images.items():
        for s in ("huffman", "rle", "auto"):
            arms[f"device_{key}_{s}"] = lambda img=img, bgr=bgr, s=s: post.encode_png(img, bgr=bgr, strategy=s)
        if a.parent_lib:
            parent = LibPngOps(a.parent_lib)
            arms[f"device_{key}_huffman_parent"] = lambda img=img, bgr=bgr, parent=parent: post.encode_png(img, bgr=bgr, ops=parent)
    size, times = {}, {k: [] for k in arms}
    for _ in range(3):                                       # warm-up
        for k, f in arms.items():
            size[k] = len(f())
    for _ in range(a.reps):
        for k, f in arms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            times[k].append((time.perf_counter() - t0) * 1e3)
    res = {k: {"median_ms": round(float(np.median(t)), 3), "min_ms": round(min(t), 3), "max_ms": round(max(t), 3), "file_bytes": size[k]}
           for k, t in times.items()}
    if a.parent_lib:
        for key in images:
            assert size[f"device_{key}_huffman_parent"] == size[f"device_{key}_huffman"]
    res["note"] = f"one MI355X, one box, {a.reps} interleaved repetitions after warm-up, {H}x{W} fixture"
    print(json.dumps(res, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
