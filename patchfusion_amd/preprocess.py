"""Device-side input preparation: what the reference's dataset does on the CPU between the
decoded uint8 image and the two tensors the model consumes.

Mirrors ``read_image`` (estimator/datasets/general_dataset.py:22-47) *after the decode* and the tensor part of
``ImageDataset.__getitem__`` (:188-219): ``img / 255.0`` (float64) -> bicubic ``align_corners=True`` resize to
``image_resolution`` -> ``to_tensor(...).float()`` = ``image_hr`` [3,H,W]; ``image_lr`` = bilinear
``align_corners=True`` resize of ``image_hr`` to the network input (depth_anything/transform.py:127-129).
The uint8 image is uploaded once (3 bytes / pixel instead of the 12 bytes / pixel float image the reference moves
with ``.cuda()``), both resizes run as HIP kernels.  There is no CPU path.
"""
import ctypes as C
import os

import numpy as np
import torch

from . import _lib

# Defaults of decode_jpeg, chosen by tools/jpeg_decode_time.py (profiles/jpeg_decode_time.json, one MI355X): at 3840x2160 (q90, 4:2:0) the
# device entropy path takes 2.5 ms at 1024-bit subsequences (3.5 ms at 256, 3.3 ms at 4096) against 35.2 ms for the host entropy path and
# 40.7 ms for PIL + upload, so the device path and 1024 bits are the defaults.  The round cap is four times the largest round count seen at
# 1024 bits on those files (12) and on the fixture (121, the 256x256 q100 noise file, which never self-synchronises).
JPEG_SUBSEQUENCE_BITS = 1024
JPEG_MAX_SYNC_ROUNDS = 484


JPEG_TABLE_WORDS, JPEG_E_STREAM, JPEG_NOT_CONVERGED = 2152, 48, 64      # PF_JPEG_TABLE_WORDS, PF_JPEG_E_STREAM, PF_JPEG_NOT_CONVERGED of pf_hip.h


class JpegError(ValueError):
    """a JPEG file decode_jpeg refuses or cannot decode; .code is the PF_JPEG_E_* status of include/pf_hip.h"""

    def __init__(self, code, what):
        super().__init__(f"jpeg: {what}")
        self.code = code


def _refusal(name, what):
    return type(name, (JpegError,), {"__doc__": what})


JPEG_ERRORS = {
    32: _refusal("JpegNotJpeg", "not a JPEG file (no SOI marker)"),
    33: _refusal("JpegTruncated", "the file ends inside its headers"),
    34: _refusal("JpegProgressive", "progressive JPEG (SOF2) is not supported: decode it on the host"),
    35: _refusal("JpegArithmetic", "arithmetic-coded JPEG is not supported"),
    36: _refusal("JpegLossless", "lossless or hierarchical JPEG is not supported"),
    37: _refusal("JpegPrecision", "only 8-bit samples are supported (12-bit file)"),
    38: _refusal("JpegQuant16", "16-bit quantisation tables are not supported"),
    39: _refusal("JpegComponents", "only 1 (grey) or 3 (YCbCr) components are supported"),
    40: _refusal("JpegColorspace", "only YCbCr colour is supported (Adobe transform or RGB component ids say otherwise)"),
    41: _refusal("JpegSampling", "only 4:4:4, 4:2:2 and 4:2:0 sampling are supported"),
    42: _refusal("JpegMultiscan", "only one interleaved scan is supported"),
    43: _refusal("JpegDnl", "DNL marker or a height of 0 is not supported"),
    44: _refusal("JpegMarker", "a marker stands where none may"),
    45: _refusal("JpegRestart", "restart markers out of sequence or count"),
    46: _refusal("JpegNoEoi", "no EOI marker after the scan"),
    47: _refusal("JpegTable", "missing or invalid Huffman or quantisation table"),
    JPEG_E_STREAM: _refusal("JpegStream", "the entropy-coded data does not decode to the frame"),
    49: _refusal("JpegScan", "the scan header is not one full sequential scan"),
}


def _jpeg_check(rc, step):
    if rc == 0:
        return
    if rc in JPEG_ERRORS:
        cls = JPEG_ERRORS[rc]
        raise cls(rc, cls.__doc__)
    raise JpegError(rc, f"{step} failed (status {rc})")


class JpegInfo:
    """what decode_jpeg reports next to the image"""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def __repr__(self):
        return "JpegInfo(" + ", ".join(f"{k}={v!r}" for k, v in self.__dict__.items()) + ")"


class JpegHost:
    """the HOST ONLY steps of the JPEG decoder (csrc/jpeg_host.h through the C ABI): no GPU call"""

    def __init__(self, data):
        self.lib = _lib.load()
        self.data = np.frombuffer(bytes(data), dtype=np.uint8)
        self.header = _lib.JpegHeader()
        _jpeg_check(self.lib.pf_jpeg_parse(self.data.ctypes.data, self.data.size, C.byref(self.header)), "pf_jpeg_parse")
        h = self.header
        cap = self.data.size - h.scan_begin + 68
        scan = np.zeros(cap, dtype=np.uint8)
        self.segs = np.zeros((h.nsegments, 2), dtype=np.uint32)
        n = C.c_long()
        _jpeg_check(self.lib.pf_jpeg_prepare_scan(self.data.ctypes.data, self.data.size, C.byref(h), scan.ctypes.data, cap, C.byref(n),
                                                  self.segs.ctypes.data), "pf_jpeg_prepare_scan")
        self.scan = scan[:n.value]

    def decode_entropy(self):
        """the sequential entropy decoder -> int16 [nblocks, 64]"""
        coef = np.zeros((self.header.nblocks, 64), dtype=np.int16)
        _jpeg_check(self.lib.pf_jpeg_decode_entropy_host(C.byref(self.header), self.scan.ctypes.data, self.scan.size, self.segs.ctypes.data,
                                                         coef.ctypes.data), "pf_jpeg_decode_entropy_host")
        return coef

    def plan(self, subsequence_bits):
        """-> (lanes uint32 [nlanes,3], segx uint32 [nsegments,4], longest segment in lanes)"""
        nl, longest = C.c_int(), C.c_int()
        S = int(subsequence_bits)
        if S < 32 or S % 32 or S > (1 << 20):
            raise ValueError(f"subsequence_bits must be a multiple of 32 in 32 .. 2^20, got {subsequence_bits}")
        _jpeg_check(self.lib.pf_jpeg_plan(C.byref(self.header), self.segs.ctypes.data, S, None, 0, None, C.byref(nl), C.byref(longest)), "pf_jpeg_plan")
        lanes = np.zeros((nl.value, 3), dtype=np.uint32)
        segx = np.zeros((self.header.nsegments, 4), dtype=np.uint32)
        _jpeg_check(self.lib.pf_jpeg_plan(C.byref(self.header), self.segs.ctypes.data, S, lanes.ctypes.data, nl.value, segx.ctypes.data,
                                          C.byref(nl), C.byref(longest)), "pf_jpeg_plan")
        return lanes, segx, longest.value

    def tables(self):
        t = np.zeros(JPEG_TABLE_WORDS, dtype=np.uint32)
        _jpeg_check(self.lib.pf_jpeg_build_tables(C.byref(self.header), t.ctypes.data), "pf_jpeg_build_tables")
        return t


def jpeg_entropy_device(host, ops, device, subsequence_bits, max_sync_rounds):
    """the device entropy step of decode_jpeg on a JpegHost -> (status, sync rounds, coefficients int16 [nblocks,64] on the device, bytes
    uploaded); status 0, or JPEG_NOT_CONVERGED with nothing usable in the coefficients (a broken stream raises)"""
    h = host.header
    up = lambda a, dt: torch.from_numpy(a.view(dt)).to(device)           # noqa: E731
    lanes, segx, longest = host.plan(subsequence_bits)
    tables = host.tables()
    coef = torch.empty((h.nblocks, 64), dtype=torch.int16, device=device)
    ws = torch.empty(ops.jpeg_workspace(h, lanes.shape[0])[0], dtype=torch.uint8, device=device)
    rc, rounds = ops.jpeg_decode_entropy(h, up(host.scan, np.uint8), up(lanes, np.int32), up(segx, np.int32), longest, up(tables, np.int32),
                                         max_sync_rounds, ws, coef)
    if rc != JPEG_NOT_CONVERGED:
        _jpeg_check(rc, "pf_jpeg_decode_entropy")
    return rc, rounds, coef, host.scan.nbytes + lanes.nbytes + segx.nbytes + tables.nbytes


def decode_jpeg(data, device="cuda", entropy="device", apply_orientation=True, subsequence_bits=None, max_sync_rounds=None, ops=None):
    """Baseline JPEG (bytes or a path) -> (uint8 [H,W,3] RGB device tensor, JpegInfo), bit-exact with libjpeg's defaults (islow, fancy
    upsampling): what ``cv2.imread`` + BGR->RGB gives (apply_orientation=True) or PIL (False).  entropy='device' uploads the compressed
    scan and decodes it in subsequences on the GPU; 'host' runs the sequential C decoder and uploads the coefficients.
    When the device path needs more than max_sync_rounds rounds the entropy step completes on the host path (info.entropy says so); the
    pixels are the same either way.  Unsupported files raise a JpegError subclass (a ValueError); there is no fallback to a host library."""
    if entropy not in ("device", "host"):
        raise ValueError(f"entropy must be 'device' or 'host', got {entropy!r}")
    S = JPEG_SUBSEQUENCE_BITS if subsequence_bits is None else int(subsequence_bits)
    cap = JPEG_MAX_SYNC_ROUNDS if max_sync_rounds is None else int(max_sync_rounds)
    if cap < 0:
        raise ValueError("max_sync_rounds must be >= 0")
    if S < 32 or S % 32 or S > (1 << 20):
        raise ValueError(f"subsequence_bits must be a multiple of 32 in 32 .. 2^20, got {subsequence_bits}")
    if isinstance(data, (str, os.PathLike)):
        with open(data, "rb") as f:
            data = f.read()
    if not isinstance(data, (bytes, bytearray, memoryview)):
        raise ValueError(f"decode_jpeg expects bytes or a path, got {type(data).__name__}")
    if ops is None:
        from .hip_ops import ops as _ops        # fails loudly when the HIP extension is missing
        ops = _ops
    dev = torch.device(device)
    host = JpegHost(data)
    h = host.header
    used, rounds, uploaded, coef = entropy, 0, 0, None
    if entropy == "device":
        rc, rounds, coef, uploaded = jpeg_entropy_device(host, ops, dev, S, cap)
        if rc == JPEG_NOT_CONVERGED:
            used = "host"                        # round cap exceeded: same coefficients from the sequential decoder
    if used == "host":
        c = host.decode_entropy()
        uploaded += c.nbytes
        coef = torch.from_numpy(c).to(dev)
    o = h.orientation if apply_orientation else 1
    H, W = (h.width, h.height) if o >= 5 else (h.height, h.width)
    rgb = torch.empty((H, W, 3), dtype=torch.uint8, device=dev)
    ops.jpeg_reconstruct(h, coef, o, torch.empty(ops.jpeg_workspace(h, 0)[1], dtype=torch.uint8, device=dev), rgb)
    info = JpegInfo(width=h.width, height=h.height, components=h.ncomp, sampling=(h.hmax, h.vmax), restart_interval=h.restart_interval,
                    orientation=h.orientation, entropy=used, sync_rounds=rounds, subsequence_bits=S, bytes_uploaded=uploaded)
    return rgb, info


class ImagePreprocessor:
    def __init__(self, image_resolution=(2160, 3840), process_shape=(392, 518), dataset_name="general", device="cuda", ops=None):
        if ops is None:
            from .hip_ops import ops as _ops        # fails loudly when the HIP extension is missing
            ops = _ops
        self.ops = ops
        self.image_resolution = tuple(int(v) for v in image_resolution)
        self.process_shape = tuple(int(v) for v in process_shape)
        self.dataset_name = dataset_name
        self.device = torch.device(device)

    def __call__(self, img_u8):
        """img_u8: decoded image, uint8 [H,W,3] (numpy or torch; RGB - or the raw BGR file order for dataset 'u4k',
        general_dataset.py:24-25) -> dict(image_hr [3,H',W'] f32, image_lr [3,h,w] f32) on the device."""
        if isinstance(img_u8, np.ndarray):
            img_u8 = torch.from_numpy(np.ascontiguousarray(img_u8))
        if img_u8.dtype != torch.uint8 or img_u8.dim() != 3 or img_u8.shape[2] != 3:
            raise ValueError(f"expected a uint8 [H,W,3] image, got {img_u8.dtype} {tuple(img_u8.shape)}")
        img_u8 = img_u8.to(self.device, non_blocking=True).contiguous()
        u4k = self.dataset_name == "u4k"
        H, W = (img_u8.shape[0], img_u8.shape[1]) if u4k else self.image_resolution   # 'u4k' raw files are never resized
        image_hr = torch.empty((3, H, W), dtype=torch.float32, device=self.device)
        self.ops.u8_bicubic_to_f32(img_u8, image_hr, reverse_channels=u4k)
        image_lr = torch.empty((3,) + self.process_shape, dtype=torch.float32, device=self.device)
        for c in range(3):
            self.ops.resize_bilinear_f32(image_hr[c], image_lr[c])
        return {"image_hr": image_hr, "image_lr": image_lr}

    def read(self, path_or_bytes, **kw):
        """decode_jpeg followed by __call__: the file never becomes a host array.  The EXIF orientation is applied for the datasets the
        reference reads with cv2.imread ('mid', general) and not for 'cityscapes', which it reads with PIL (no rotation).  'u4k' files are
        raw arrays, not JPEG: refused."""
        if self.dataset_name == "u4k":
            raise ValueError("dataset 'u4k' stores raw arrays, not JPEG files: there is nothing to decode")
        kw.setdefault("apply_orientation", self.dataset_name != "cityscapes")
        rgb, self.last_jpeg_info = decode_jpeg(path_or_bytes, device=self.device, ops=self.ops, **kw)
        return self(rgb)
