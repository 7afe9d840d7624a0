"""Numpy restatement of the reference's ground-truth loaders, for tests/test_gt_*.py and tools/gt_read_time.py (TEST INFRASTRUCTURE
ONLY): file bytes in, float32 depth, edge source and edges out.

  read_pfm     estimator/datasets/utils.py:5-49 readPFM
  depth_map    estimator/datasets/general_dataset.py:60-143 DepthMap ('u4k' is also u4k_dataset.py:118-119,168)

Written from the arithmetic table of the ground-truth reader (include/pf_hip.h): a Python float that meets a float32 array is
rounded to float32 first, every +, - and / is one float32 operation.  Pinned bit for bit to the reference's own classes in
tests/test_gt_ref_cpu.py (live, and against tests/golden/gt_readers.npz).  Boundaries reuse tests/eval_side_ref.py.  PNG samples come
from tests/png_decode_ref.py, the stand-in for imageio.imread / cv2.imread(IMREAD_UNCHANGED) on a grey file.

The second half builds the files and the seeded inputs the CPU and GPU modules share."""
import io
import re

import numpy as np

from tests import eval_side_ref as E
from tests import png_decode_ref as P

DATASETS = ("u4k", "gta", "eth3d", "mid", "cityscapes")
F32 = np.float32


def same_bits(a, b):
    """equal bit patterns, NaNs matching NaNs whatever their sign or payload"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype != np.float32 or b.dtype != np.float32 or a.shape != b.shape:
        return False
    nan = np.isnan(a)
    return bool(np.array_equal(nan, np.isnan(b)) and np.array_equal(a.view(np.uint32)[~nan], b.view(np.uint32)[~nan]))


# ---------------------------------------------------------------- the loaders
def read_pfm(data):
    """-> (float array [H,W] or [H,W,3] in the FILE's byte order, top row first; scale)"""
    f = io.BytesIO(bytes(data))
    header = f.readline().rstrip().decode("utf-8")
    if header not in ("PF", "Pf"):
        raise ValueError(f"magic {header!r} is neither Pf nor PF")
    dims = re.match(r"^(\d+)\s(\d+)\s$", f.readline().decode("utf-8"))
    if not dims:
        raise ValueError("the dimension line does not match")
    width, height = map(int, dims.groups())
    scale = float(f.readline().rstrip().decode("utf-8"))
    endian = "<" if scale < 0 else ">"
    a = np.frombuffer(f.read(), dtype=endian + "f")
    return np.flipud(a.reshape((height, width, 3) if header == "PF" else (height, width))), abs(scale) if scale < 0 else scale


def read_npy(data):
    with np.errstate(over="ignore"):                             # a double beyond float32's range is inf
        return np.load(io.BytesIO(bytes(data))).astype(F32)


def parse_calib(text):
    lines = text.splitlines(True)
    f = float(lines[0].strip().split(" ")[0].split("[")[1])
    return f, float(lines[2].strip().split("=")[1]), float(lines[3].strip().split("=")[1])      # f, doffs, baseline


def nan_to_zero(a):
    a = a.copy()
    a[~np.isfinite(a)] = 0
    return a


def planes(dataset, data, depth_factor=None, calib=None, shape=(4032, 6048)):
    """-> (depth, edge source) float32"""
    with np.errstate(all="ignore"):
        if dataset == "u4k":
            x = read_npy(data)
            while x.ndim > 2 and x.shape[0] == 1:                # unit axes at either end: the reader squeezes them
                x = x[0]
            while x.ndim > 2 and x.shape[-1] == 1:
                x = x[..., 0]
            return F32(depth_factor) / x, x
        if dataset == "mid":
            f, doffs, base = parse_calib(calib) if isinstance(calib, str) else calib
            x = read_pfm(data)[0].astype(F32)
            invalid = x == np.inf
            depth = (F32(base * f) / (x + F32(doffs))) / F32(1000)
            depth[invalid] = 0
            edge = x.copy()
            edge[invalid] = 0
            return depth, edge
        if dataset == "eth3d":
            d = nan_to_zero(np.frombuffer(bytes(data), dtype="<f4").reshape(shape).astype(F32))
            return d, d
        if dataset == "gta":
            d = P.decode(bytes(data)).astype(F32) / F32(256)
            return d, d
        if dataset == "cityscapes":
            s = P.decode(bytes(data)).astype(F32)
            pos = s > 0
            s[pos] = (s[pos] - F32(1)) / F32(256)
            d = nan_to_zero(F32(0.209313 * 2262.52) / s)
            return d, d
    raise NotImplementedError(dataset)


def depth_map(dataset, data, depth_factor=None, calib=None, shape=(4032, 6048), th=1.0, dilation=0):
    """-> (depth, edge source, edges), all float32 [H,W]"""
    depth, edge_source = planes(dataset, data, depth_factor, calib, shape)
    assert depth.dtype == F32 and edge_source.dtype == F32
    with np.errstate(all="ignore"):                              # max - (-max) overflows to inf: an edge, as in the reference
        return depth, edge_source, E.get_boundaries(edge_source, th, dilation)


# ---------------------------------------------------------------- file writers
def npy_bytes(a, version=(1, 0), shape=None, fortran=False, descr=None):
    """an .npy file of `a` written by hand (numpy's writer picks the version itself): magic, version, header length, dict, payload"""
    a = np.asarray(a)
    d = "{'descr': %r, 'fortran_order': %r, 'shape': %r, }" % (descr or a.dtype.str, fortran, tuple(a.shape if shape is None else shape))
    head = d.encode("utf-8" if version == (3, 0) else "latin1")
    pre = 10 if version == (1, 0) else 12
    head += b" " * (-(pre + len(head) + 1) % 64) + b"\n"
    n = len(head).to_bytes(2 if version == (1, 0) else 4, "little")
    return b"\x93NUMPY" + bytes(version) + n + head + a.tobytes()


def pfm_bytes(a, little=True, scale=1.0, colour=False):
    """`a` is the image top row first ([H,W] or [H,W,3]); the file stores the bottom row first"""
    a = np.asarray(a)
    H, W = a.shape[:2]
    s = -abs(scale) if little else abs(scale)
    return (b"PF" if colour else b"Pf") + b"\n%d %d\n%s\n" % (W, H, repr(float(s)).encode()) + \
        np.flipud(a).astype("<f4" if little else ">f4").tobytes()


def png_bytes(samples, depth=16, filters=(0, 1, 2, 3, 4)):
    return P.write_png(np.asarray(samples), 0, depth, filters=filters)


CALIB = (3997.684, 131.111, 193.001)                             # f, doffs, baseline of a Middlebury 2014 scene


def calib_text(f=CALIB[0], doffs=CALIB[1], base=CALIB[2]):
    return (f"cam0=[{f} 0 1176.728; 0 {f} 1011.728; 0 0 1]\ncam1=[{f} 0 1307.839; 0 {f} 1011.728; 0 0 1]\ndoffs={doffs}\n"
            f"baseline={base}\nwidth=2964\nheight=1988\nndisp=280\nisint=0\nvmin=31\nvmax=257\n")


# ---------------------------------------------------------------- the reference's own classes on one case (build container only)
class _SmallEth3d:
    """stands in for `np` inside general_dataset: DepthMap reshapes an eth3d file to a hard-coded 4032 x 6048; here np.fromfile's result
    reshapes to the case's small shape whatever it is asked for.  Everything else is numpy itself."""

    def __init__(self, shape):
        self._shape = shape

    def __getattr__(self, name):
        return getattr(np, name)

    def fromfile(self, *a, **k):
        shape = self._shape

        class _Flat(np.ndarray):
            def reshape(self, *_a, **_k):
                return np.asarray(self).reshape(shape)
        return np.fromfile(*a, **k).view(_Flat)


def run_reference(case, tmp):
    """DepthMap (or readPFM for dataset 'pfm') of the reference on the case's file written under tmp -> dict of arrays.  The reference's
    readPFM uses `sys` without importing it (NameError as shipped): the module gets it set here.  cv2.imread / imageio.imread are stubs
    that return the samples the PNG was written from."""
    import os
    import sys

    from oracle import ref_shim
    ref_shim.import_reference()
    import estimator.datasets.general_dataset as g
    import estimator.datasets.utils as u
    u.sys = sys
    ds, name = case["dataset"], case["name"]
    sub, ext = {"u4k": ("val_gt", ".npy"), "mid": ("gts", ".pfm"), "pfm": ("gts", ".pfm"), "eth3d": ("eth3d", ".bin"), "gta": ("gta", ".png"),
                "cityscapes": ("cityscapes", ".png")}[ds]
    root = os.path.join(str(tmp), name, sub)
    os.makedirs(root, exist_ok=True)
    with open(os.path.join(root, "a" + ext), "wb") as f:
        f.write(case["data"])
    if ds == "pfm":
        a, scale = u.readPFM(os.path.join(root, "a.pfm"))
        return dict(pfm=np.ascontiguousarray(a.astype(F32)), scale=np.float64(scale))
    if ds in ("u4k", "mid"):
        side = root.replace("val_gt", "val_factor").replace("gts", "calibs")
        os.makedirs(side, exist_ok=True)
        with open(os.path.join(side, "a.txt"), "w") as f:
            f.write(case["side"])
    samples = P.decode(case["data"]) if ds in ("gta", "cityscapes") else None
    old = g.np, getattr(g.imageio, "imread", None), getattr(g.cv2, "imread", None), getattr(g.cv2, "IMREAD_UNCHANGED", None)
    g.imageio.imread = lambda path: samples.copy()
    g.cv2.imread = lambda path, flag=None: samples.copy()
    g.cv2.IMREAD_UNCHANGED = -1
    if ds == "eth3d":
        g.np = _SmallEth3d(case["shape"])
    try:
        with np.errstate(all="ignore"):
            m = g.DepthMap(root, ["a" + ext], 0, ds)
    finally:
        g.np, g.imageio.imread, g.cv2.imread, g.cv2.IMREAD_UNCHANGED = old
    return dict(depth=np.ascontiguousarray(m.gt), edge=np.ascontiguousarray(m.edge))


def golden_cases():
    """the cases of tests/golden/gt_readers.npz (tools/make_golden_gt.py): at most 37 x 53, inputs as file bytes"""
    cases = []
    for kind, order, version, df in (("f2", "<", (1, 0), 1234.5678), ("f4", "<", (1, 0), 1234.5678), ("f8", "<", (2, 0), 1234.5678),
                                     ("f8", ">", (3, 0), 1234.5678), ("f4", ">", (1, 0), DENORMAL_DF)):
        a = float_plane(37, 53, kind, seed=11).astype(order + kind)
        cases.append(dict(name=f"u4k_{kind}_{'be' if order == '>' else 'le'}", dataset="u4k", data=npy_bytes(a, version), side=f"{df!r}\n",
                          kwargs=dict(depth_factor=df)))
    for little in (True, False):
        cases.append(dict(name=f"mid_{'le' if little else 'be'}", dataset="mid", data=pfm_bytes(float_plane(37, 53, "f4", seed=12), little),
                          side=calib_text(), kwargs=dict(calib=calib_text())))
    cases.append(dict(name="eth3d", dataset="eth3d", data=float_plane(33, 52, "f4", seed=13).astype("<f4").tobytes(), shape=(33, 52),
                      kwargs=dict(shape=(33, 52))))
    for ds in ("gta", "cityscapes"):
        for depth in (16, 8):
            cases.append(dict(name=f"{ds}_{depth}", dataset=ds, data=png_bytes(sample_plane(29, 53, depth, 14, ds), depth), kwargs={}))
    rs = np.random.RandomState(15)
    cases.append(dict(name="pfm_colour", dataset="pfm", data=pfm_bytes(rs.randn(5, 7, 3).astype(F32), False, 0.5, colour=True), kwargs={}))
    cases.append(dict(name="pfm_grey", dataset="pfm", data=pfm_bytes(float_plane(6, 9, "f4", seed=16), True, 2.0), kwargs={}))
    return cases


# ---------------------------------------------------------------- seeded inputs
SHAPES = ((1, 1), (1, 3), (2, 53), (37, 53), (33, 64), (37, 130))
DENORMAL_DF = float(F32(1e-38))                                  # with x = 3 the quotient is a float32 denormal


def _ramp(H, W, seed):
    """a smooth plane with isolated jumps: some neighbours differ by more than 1, most do not"""
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    return 50.0 + 0.31 * xx + 0.23 * yy + (rs.rand(H, W) < 0.12) * rs.rand(H, W) * 9.0 + rs.rand(H, W) * 0.4


def _plant(a, values):
    """the planted values at the start of the plane and, reversed, at its end (the last H * W % 4 pixels take their own path)"""
    flat = a.reshape(-1)
    v = np.asarray(values, dtype=a.dtype)[:flat.size]
    flat[:v.size] = v
    flat[flat.size - v.size:] = v[::-1]
    return a


def float_plane(H, W, kind, seed):
    """disparities of dtype f2 / f4 / f8 with the planted row: zeros of both signs, infinities, NaN, the extreme normal numbers,
    denormals, 3 (denormal quotient under DENORMAL_DF), and for f8 values halfway between two floats, beyond float32's range and below it"""
    dt = np.dtype(kind)
    a = _ramp(H, W, seed).astype(dt)
    fi = np.finfo(dt)
    special = [0.0, -0.0, np.inf, -np.inf, np.nan, fi.max, -fi.max, fi.tiny, -fi.tiny, fi.tiny / 4, float(np.nextafter(dt.type(0), dt.type(1))), 3.0,
               1.0, 7.0, -3.0]
    if kind == "f8":
        for v in (F32(1.0), F32(3.1415927), F32(1e-40), F32(6.5e37), F32(2.5)):
            up, dn = np.nextafter(v, F32(np.inf)), np.nextafter(v, F32(-np.inf))
            special += [(float(v) + float(up)) / 2, (float(v) + float(dn)) / 2]          # ties: round to even
        special += [1e300, -1e300, 1e-300, 3.4028235677973366e38, 1.401298464324817e-45 / 2, 1.401298464324817e-45 * 0.75, 1e-42]
    elif kind == "f4":
        special += [1e-42, 2.9e-39, 1.1754942e-38, 3e38, 1e-30, F32(131.111) * -1, 868.889]
    with np.errstate(over="ignore"):
        return _plant(a, np.array(special, dtype=np.float64).astype(dt))


def sample_plane(H, W, depth, seed, dataset):
    """grey samples of 8 or 16 bits with 0, 1, 2, 255, 256, 65535 planted (8 bits: their low bytes)"""
    r = _ramp(H, W, seed)
    if depth == 16:
        s = (r * (256 if dataset == "gta" else 90)).astype(np.uint16)
    else:
        s = r.astype(np.uint8)
    return _plant(s, np.array([0, 1, 2, 255, 256, 65535, 3, 257, 128]).astype(s.dtype))


def metric_plane(H, W, lo, hi, seed):
    """smooth float64 values in [lo, hi] with a step: the source of a ground truth whose depth stays inside [3, 8]
    (tests/eval_side_ref.py metric_case: then every sum of the metrics kernel is exact, whatever the order of its atomics)"""
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    u = 0.3 + 0.1 * np.sin(xx / 13.0) * np.cos(yy / 9.0) + 0.4 * (xx > W // 2) + 0.04 * rs.rand(H, W)
    return lo + (hi - lo) * np.clip(u, 0.0, 1.0)
