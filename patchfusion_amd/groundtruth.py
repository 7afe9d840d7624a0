"""Ground-truth depth files read on the device (csrc/gtread.hip): the other operand of the evaluation loop.

The reference's ``DepthMap`` (estimator/datasets/general_dataset.py:60-143) and ``UnrealStereo4kDataset.__getitem__``
(u4k_dataset.py:110-178) load an 8 to 24 megapixel array on the host, make two to five numpy passes over it, then run get_boundaries.
Here the host parses the file's HEADER only (pure Python, a few dozen bytes), uploads the payload once as it lies on disk, and one HIP
launch makes the float32 depth plane and the plane get_boundaries takes, with the reference's float32 arithmetic operation by operation
(the table in include/pf_hip.h); the edges come from the existing boundary kernel.  The samples never become a host array.

Unsupported or broken files raise a GtError subclass (a ValueError); there is no fallback to numpy loading.
"""
import ast
import os
import re
import struct
import sys
import warnings

import numpy as np
import torch

DATASETS = ("u4k", "gta", "eth3d", "mid", "cityscapes")
ETH3D_SHAPE = (4032, 6048)                                     # general_dataset.py:89
CITYSCAPES_FACTOR = 0.209313 * 2262.52                         # general_dataset.py:129: baseline * focal length, the product in double


class GtError(ValueError):
    """a ground-truth file read_depth_gt / read_pfm / read_npy refuses"""

    def __init__(self, what=None):
        super().__init__(f"ground truth: {what or self.__doc__}")


def _refusal(name, what):
    return type(name, (GtError,), {"__doc__": what})


GtNpyHeader = _refusal("GtNpyHeader", "not an NPY file of version 1.0, 2.0 or 3.0, or its header does not parse")
GtNpyDtype = _refusal("GtNpyDtype", "NPY dtype is not a half, float or double (integer, object and structured arrays are refused)")
GtNpyFortran = _refusal("GtNpyFortran", "NPY array is in Fortran order")
GtNpyShape = _refusal("GtNpyShape", "NPY array is not two-dimensional (unit axes at either end aside)")
GtPfmHeader = _refusal("GtPfmHeader", "not a PFM file, or its header is malformed")
GtPfmColour = _refusal("GtPfmColour", "a three-channel PFM ('PF') is no disparity map")
GtPayloadSize = _refusal("GtPayloadSize", "the payload's size does not match the shape")
GtSideFile = _refusal("GtSideFile", "depth factor / calibration missing: with bytes as input it must be passed")
GtCalib = _refusal("GtCalib", "the calibration does not parse")
GtPngLayout = _refusal("GtPngLayout", "the PNG is not single-channel grey of 8 or 16 bits")
GtInput = _refusal("GtInput", "expected bytes or a path")


class GtInfo:
    """what read_depth_gt reports next to the planes"""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def __repr__(self):
        return "GtInfo(" + ", ".join(f"{k}={v!r}" for k, v in self.__dict__.items()) + ")"


class GroundTruth:
    """.depth float32 [H,W]; .edge float32 0/1 [H,W] or None; .edge_source: the plane get_boundaries took; .info"""

    def __init__(self, depth, edge, edge_source, info):
        self.depth, self.edge, self.edge_source, self.info = depth, edge, edge_source, info


# ---------------------------------------------------------------- host side: headers only
def _bytes_of(path_or_bytes):
    """-> (bytes-like, path or None)"""
    if isinstance(path_or_bytes, (str, os.PathLike)):
        with open(path_or_bytes, "rb") as f:
            return f.read(), os.fspath(path_or_bytes)
    if isinstance(path_or_bytes, (bytes, bytearray, memoryview)):
        return path_or_bytes, None
    raise GtInput(f"expected bytes or a path, got {type(path_or_bytes).__name__}")


def parse_npy(data):
    """NPY header -> (kind 'f2' | 'f4' | 'f8', byte order '<' | '>', (H, W), payload offset, version).  numpy/lib/format.py's layout:
    magic, two version bytes, a little-endian header length of 2 (version 1) or 4 bytes, a Python dict literal."""
    head = bytes(data[:12])
    if len(head) < 10 or head[:6] != b"\x93NUMPY":
        raise GtNpyHeader()
    version = (head[6], head[7])
    if version == (1, 0):
        hlen, start = struct.unpack("<H", head[8:10])[0], 10
    elif version in ((2, 0), (3, 0)) and len(head) == 12:
        hlen, start = struct.unpack("<I", head[8:12])[0], 12
    else:
        raise GtNpyHeader(f"NPY version {version[0]}.{version[1]} is not supported")
    if start + hlen > len(data):
        raise GtNpyHeader("the NPY header runs past the file")
    try:
        d = ast.literal_eval(bytes(data[start:start + hlen]).decode("utf-8" if version == (3, 0) else "latin1"))
        descr, fortran, shape = d["descr"], d["fortran_order"], d["shape"]
    except Exception:
        raise GtNpyHeader() from None
    if not isinstance(descr, str) or len(descr) != 3 or descr[0] not in "<>=|" or descr[1:] not in ("f2", "f4", "f8"):
        raise GtNpyDtype(f"NPY dtype {descr!r}: only <f2 <f4 <f8 >f2 >f4 >f8 are read")
    if fortran is not False:
        raise GtNpyFortran()
    if not isinstance(shape, tuple) or not all(isinstance(v, int) and not isinstance(v, bool) for v in shape):
        raise GtNpyHeader()
    shape = list(shape)
    while len(shape) > 2 and shape[0] == 1:
        shape.pop(0)
    while len(shape) > 2 and shape[-1] == 1:
        shape.pop()
    if len(shape) != 2 or shape[0] <= 0 or shape[1] <= 0:
        raise GtNpyShape(f"NPY shape {d['shape']} is not two-dimensional")
    order = descr[0] if descr[0] in "<>" else ("<" if sys.byteorder == "little" else ">")
    kind = descr[1:]
    need = shape[0] * shape[1] * int(kind[1])
    if len(data) - (start + hlen) < need:
        raise GtPayloadSize(f"the NPY payload holds {len(data) - start - hlen} bytes, the header promises {need}")
    return kind, order, (shape[0], shape[1]), start + hlen, version


_PFM_DIMS = re.compile(r"^(\d+)\s(\d+)\s$")


def parse_pfm(data):
    """PFM header as estimator/datasets/utils.py:5-49 reads it -> (colour, (H, W), scale, byte order, payload offset): three
    readline()s, 'Pf' or 'PF', the reference's own dimension pattern, the sign of the scale selecting the byte order (negative: little
    endian); the rest of the file is the payload and must hold exactly H * W (* 3) floats."""
    lines, pos = [], 0
    view = bytes(data[:256])
    for _ in range(3):
        nl = view.find(b"\n", pos)
        end = len(view) if nl < 0 else nl + 1
        lines.append(view[pos:end])
        pos = end
    try:
        magic = lines[0].rstrip().decode("utf-8")
        dims = _PFM_DIMS.match(lines[1].decode("utf-8"))
        scale = float(lines[2].rstrip().decode("utf-8"))
    except (UnicodeDecodeError, ValueError):
        raise GtPfmHeader() from None
    if magic not in ("PF", "Pf"):
        raise GtPfmHeader("not a PFM file")
    if not dims:
        raise GtPfmHeader("malformed PFM header")
    W, H = int(dims.group(1)), int(dims.group(2))
    if H <= 0 or W <= 0:
        raise GtPfmHeader("malformed PFM header: empty image")
    colour = magic == "PF"
    order = "<" if scale < 0 else ">"
    need = 4 * H * W * (3 if colour else 1)
    if len(data) - pos != need:
        raise GtPayloadSize(f"the PFM payload holds {len(data) - pos} bytes, {W} x {H}{' x 3' if colour else ''} floats need {need}")
    return colour, (H, W), abs(scale) if scale < 0 else scale, order, pos


def parse_calib(text):
    """Middlebury calibration text -> (f, doffs, baseline), general_dataset.py:102-107: the focal length is the first number of the
    matrix on line 0, doffs on line 2 and the baseline on line 3, each after '='."""
    try:
        lines = text.splitlines(True)
        f = float(lines[0].strip().split(" ")[0].split("[")[1])
        base = float(lines[3].strip().split("=")[1])
        doffs = float(lines[2].strip().split("=")[1])
    except (IndexError, ValueError):
        raise GtCalib() from None
    return f, doffs, base


def u4k_factor_path(gt_path):
    return gt_path.replace("val_gt", "val_factor").replace(".npy", ".txt")        # general_dataset.py:67-68


def mid_calib_path(gt_path):
    return gt_path.replace("gts", "calibs").replace(".pfm", ".txt")               # general_dataset.py:100-101


def _depth_factor(depth_factor, path):
    if depth_factor is None:
        if path is None:
            raise GtSideFile("with bytes as input depth_factor must be passed")
        with open(u4k_factor_path(path), "r") as f:
            depth_factor = f.readline()
    try:
        return float(depth_factor)
    except (TypeError, ValueError):
        raise GtCalib(f"the depth factor {depth_factor!r} is no number") from None


def _calibration(calib, path):
    if calib is None:
        if path is None:
            raise GtSideFile("with bytes as input calib must be passed")
        with open(mid_calib_path(path), "r") as f:
            calib = f.read()
    if isinstance(calib, (bytes, bytearray)):
        calib = bytes(calib).decode("utf-8")
    if isinstance(calib, str):
        return parse_calib(calib)
    try:
        f, doffs, base = (float(v) for v in calib)
    except (TypeError, ValueError):
        raise GtCalib("calib is (f, doffs, baseline) or the text of the calibration file") from None
    return f, doffs, base


# ---------------------------------------------------------------- device side
def _ops(ops):
    if ops is None:
        from .hip_ops import ops as _o          # fails loudly when the HIP extension is missing
        return _o
    return ops


def _upload(data, offset, nbytes, dev):
    """the payload, from its own offset, as a uint8 device tensor: the device buffer starts at the first sample"""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)               # "buffer is not writable": it is only read
        host = torch.frombuffer(data, dtype=torch.uint8, count=nbytes, offset=offset)
    return host.to(dev)


def _f32(v):
    """a Python float as numpy rounds it when it meets a float32 array"""
    with np.errstate(over="ignore"):
        return float(np.float32(v))


def _planes(ops, dev, src, kind, mode, shape, a=0.0, b=0.0, own_edge=False, swap=False, flip=False):
    depth = torch.empty(shape, dtype=torch.float32, device=dev)
    edge_source = torch.empty(shape, dtype=torch.float32, device=dev) if own_edge else None
    ops.gt_convert(src, kind, mode, shape[0], shape[1], _f32(a), _f32(b), depth, edge_source, swap=swap, flip=flip)
    return depth, depth if edge_source is None else edge_source


def read_npy(path_or_bytes, device="cuda", ops=None):
    """.npy of halves, floats or doubles -> float32 [H,W] on the device: np.load(...).astype(np.float32)"""
    data, _ = _bytes_of(path_or_bytes)
    kind, order, shape, off, _ = parse_npy(data)
    dev = torch.device(device)
    src = _upload(data, off, shape[0] * shape[1] * int(kind[1]), dev)
    return _planes(_ops(ops), dev, src, kind, "raw", shape, swap=order == ">")[0]


def read_pfm(path_or_bytes, device="cuda", ops=None):
    """readPFM (estimator/datasets/utils.py:5-49) on the device -> (float32 [H,W] or [H,W,3], top row first; scale)"""
    data, _ = _bytes_of(path_or_bytes)
    colour, (H, W), scale, order, off = parse_pfm(data)
    dev = torch.device(device)
    ch = 3 if colour else 1
    src = _upload(data, off, 4 * H * W * ch, dev)
    plane = _planes(_ops(ops), dev, src, "f4", "raw", (H, W * ch), swap=order == ">", flip=True)[0]
    return (plane.view(H, W, 3) if colour else plane), scale


def read_depth_gt(path_or_bytes, dataset_name, *, depth_factor=None, calib=None, shape=None, device="cuda", edges=True, th=1.0, dilation=0,
                  png_options=None, ops=None):
    """One ground-truth file of `dataset_name` ('u4k' | 'gta' | 'eth3d' | 'mid' | 'cityscapes'; anything else NotImplementedError, as
    general_dataset.py:138-139) -> GroundTruth(depth, edge, edge_source, info), every plane float32 [H,W] on the device and equal to
    DepthMap's `gt` / `edge` bit for bit.
      u4k         .npy disparity; depth_factor or, from a path, the first line of the val_gt -> val_factor, .npy -> .txt file
      mid         .pfm disparity; calib = (f, doffs, baseline) or the calibration text or, from a path, the gts -> calibs, .pfm -> .txt file
      eth3d       raw little-endian float32 of `shape` (default 4032 x 6048)
      gta         grey PNG of 8 or 16 bits through decode_png(**png_options)
      cityscapes  the same
    edges=True runs get_boundaries(edge_source, th, dilation) (the reference's th = 1, dilation = 0); edges=False leaves .edge None."""
    if dataset_name not in DATASETS:
        raise NotImplementedError(f"dataset {dataset_name!r}")
    data, path = _bytes_of(path_or_bytes)
    ops = _ops(ops)
    dev = torch.device(device)
    info = dict(dataset=dataset_name, scale=None)
    if dataset_name == "u4k":
        kind, order, shape, off, version = parse_npy(data)
        df = _depth_factor(depth_factor, path)
        nbytes = shape[0] * shape[1] * int(kind[1])
        depth, edge_source = _planes(ops, dev, _upload(data, off, nbytes, dev), kind, "u4k", shape, a=df, own_edge=True, swap=order == ">")
        info.update(format="npy", npy_version=version, dtype=kind, endianness=order, depth_factor=df, bytes_uploaded=nbytes)
    elif dataset_name == "mid":
        colour, shape, scale, order, off = parse_pfm(data)
        if colour:
            raise GtPfmColour()
        f, doffs, base = _calibration(calib, path)
        nbytes = 4 * shape[0] * shape[1]
        depth, edge_source = _planes(ops, dev, _upload(data, off, nbytes, dev), "f4", "mid", shape, a=base * f, b=doffs, own_edge=True,
                                     swap=order == ">", flip=True)
        info.update(format="pfm", dtype="f4", endianness=order, scale=scale, calib=(f, doffs, base), bytes_uploaded=nbytes)
    elif dataset_name == "eth3d":
        shape = ETH3D_SHAPE if shape is None else (int(shape[0]), int(shape[1]))
        nbytes = 4 * shape[0] * shape[1]
        if shape[0] <= 0 or shape[1] <= 0 or len(data) != nbytes:
            raise GtPayloadSize(f"the file holds {len(data)} bytes, {shape[0]} x {shape[1]} floats need {nbytes}")
        depth, edge_source = _planes(ops, dev, _upload(data, 0, nbytes, dev), "f4", "eth3d", shape)
        info.update(format="raw", dtype="f4", endianness="<", bytes_uploaded=nbytes)
    else:
        from .preprocess import decode_png
        image, png = decode_png(data, device=dev, ops=ops, **(png_options or {}))
        if image.dim() != 2 or png.color_type != 0 or png.bit_depth not in (8, 16):
            raise GtPngLayout(f"the PNG has colour type {png.color_type} and {png.bit_depth} bits: single-channel grey of 8 or 16 bits is read")
        shape = tuple(image.shape)
        kind = "u2" if png.bit_depth == 16 else "u1"
        depth, edge_source = _planes(ops, dev, image, kind, dataset_name, shape, a=CITYSCAPES_FACTOR if dataset_name == "cityscapes" else 0.0)
        info.update(format="png", dtype=kind, endianness=None, bytes_uploaded=png.bytes_uploaded, png=png)
    edge = None
    if edges:
        edge = ops.depth_boundaries(edge_source, th, dilation, torch.empty_like(edge_source))
    info.update(shape=tuple(shape), path=path)
    return GroundTruth(depth, edge, edge_source, GtInfo(**info))
