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
# Progressive files (progressive=True; tools/jpeg_prog_decode_time.py, profiles/jpeg_prog_decode_time.json) keep both defaults: 256 and 1024
# bits are within 6 % of each other there with no consistent order (36.9 ms at 1024 bits at 3840x2160 against 73.2 ms for PIL + upload and
# 62.2 ms for the host entropy path), 4096 is slower on every file, and the host's AC refinement, not the rounds, is 73-89 % of the time.
JPEG_SUBSEQUENCE_BITS = 1024
JPEG_MAX_SYNC_ROUNDS = 484


JPEG_TABLE_WORDS, JPEG_E_STREAM, JPEG_NOT_CONVERGED = 2152, 48, 64      # PF_JPEG_TABLE_WORDS, PF_JPEG_E_STREAM, PF_JPEG_NOT_CONVERGED of pf_hip.h
JPEG_PROG_BASELINE = 65                                                 # PF_JPEG_PROG_BASELINE
JPEG_PROG_KINDS = ("dc_first", "dc_refine", "ac_first", "ac_refine")    # PF_JPEG_PROG_DC_FIRST .. PF_JPEG_PROG_AC_REFINE


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
    # progressive files (decode_jpeg(..., progressive=True))
    50: _refusal("JpegProgNoFirst", "progressive: a scan refines a coefficient that had no first scan"),
    51: _refusal("JpegProgAh", "progressive: a scan's Ah is not the Al the coefficient was last sent at"),
    52: _refusal("JpegProgAl", "progressive: a refinement scan with Al other than Ah - 1"),
    53: _refusal("JpegProgAcComponents", "progressive: an AC scan with more than one component"),
    54: _refusal("JpegProgAcBeforeDc", "progressive: an AC scan before its component's DC scan"),
    55: _refusal("JpegProgBand", "progressive: a scan's band is not Ss <= Se <= 63 (Se = 0 for a DC scan)"),
    56: _refusal("JpegProgIncomplete", "progressive: the progression is incomplete (a coefficient never sent, or not refined to bit 0); "
                                       "libjpeg would smooth such a file, which is not reproduced"),
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


class JpegProgHost:
    """the HOST ONLY steps of the progressive decoder (csrc/jpeg_host.h through the C ABI): no GPU call.  .baseline is True for a baseline
    file (nothing else is set then: use JpegHost)."""

    def __init__(self, data):
        self.lib = _lib.load()
        raw = bytes(data)
        self.data = np.frombuffer(raw, dtype=np.uint8)
        self.header = _lib.JpegHeader()
        cap = raw.count(b"\xff\xda") + 1                     # every SOS is such a pair
        arr = (_lib.JpegProgScan * cap)()
        n = C.c_int()
        rc = self.lib.pf_jpeg_prog_parse(self.data.ctypes.data, self.data.size, C.byref(self.header), arr, cap, C.byref(n))
        self.baseline = rc == JPEG_PROG_BASELINE
        if not self.baseline:
            _jpeg_check(rc, "pf_jpeg_prog_parse")
        self.scans = [arr[i] for i in range(n.value)]
        self._keep = arr

    def prepare(self, scan):
        """-> (the scan's unstuffed bytes, zero-padded; segs uint32 [nsegments, 2])"""
        cap = scan.end - scan.begin + 68
        out = np.zeros(cap, dtype=np.uint8)
        segs = np.zeros((scan.nsegments, 2), dtype=np.uint32)
        n = C.c_long()
        _jpeg_check(self.lib.pf_jpeg_prog_prepare_scan(self.data.ctypes.data, self.data.size, C.byref(scan), out.ctypes.data, cap, C.byref(n),
                                                       segs.ctypes.data), "pf_jpeg_prog_prepare_scan")
        return out[:n.value], segs

    def decode_scan(self, scan, coef, prepared=None):
        """the sequential decoder of one scan applied to coef int16 [nblocks, 64]"""
        data, segs = prepared or self.prepare(scan)
        _jpeg_check(self.lib.pf_jpeg_prog_decode_scan_host(C.byref(self.header), C.byref(scan), data.ctypes.data, data.size, segs.ctypes.data,
                                                           coef.ctypes.data), "pf_jpeg_prog_decode_scan_host")

    def decode_entropy(self):
        """every scan through the sequential decoder -> int16 [nblocks, 64]"""
        coef = np.zeros((self.header.nblocks, 64), dtype=np.int16)
        for scan in self.scans:
            self.decode_scan(scan, coef)
        return coef

    def refine_ac(self, scan, masks, prepared=None):
        """an AC-refinement scan against masks uint64 [scan blocks] (updated in place) -> records uint64 [scan blocks, 3]"""
        data, segs = prepared or self.prepare(scan)
        assert masks.dtype == np.uint64 and masks.flags.c_contiguous and masks.size == scan.nblocks
        rec = np.zeros((scan.nblocks, 3), dtype=np.uint64)
        _jpeg_check(self.lib.pf_jpeg_prog_refine_ac_host(C.byref(scan), data.ctypes.data, data.size, segs.ctypes.data, masks.ctypes.data,
                                                         rec.ctypes.data), "pf_jpeg_prog_refine_ac_host")
        return rec

    def plan(self, scan, segs, subsequence_bits):
        nl, longest = C.c_int(), C.c_int()
        S = int(subsequence_bits)
        _jpeg_check(self.lib.pf_jpeg_prog_plan(C.byref(scan), segs.ctypes.data, S, None, 0, None, C.byref(nl), C.byref(longest)), "pf_jpeg_prog_plan")
        lanes = np.zeros((nl.value, 3), dtype=np.uint32)
        segx = np.zeros((scan.nsegments, 4), dtype=np.uint32)
        _jpeg_check(self.lib.pf_jpeg_prog_plan(C.byref(scan), segs.ctypes.data, S, lanes.ctypes.data, nl.value, segx.ctypes.data, C.byref(nl),
                                               C.byref(longest)), "pf_jpeg_prog_plan")
        return lanes, segx, longest.value

    def tables(self, scan):
        t = np.zeros(JPEG_TABLE_WORDS, dtype=np.uint32)
        _jpeg_check(self.lib.pf_jpeg_prog_build_tables(C.byref(scan), t.ctypes.data), "pf_jpeg_prog_build_tables")
        return t

    def block_map(self, scan):
        """int32 [scan blocks]: where each block of a one-component scan's raster walk lies in the coefficient array"""
        m = np.zeros(scan.nblocks, dtype=np.int32)
        _jpeg_check(self.lib.pf_jpeg_prog_block_map(C.byref(self.header), C.byref(scan), m.ctypes.data), "pf_jpeg_prog_block_map")
        return m


def _scan_entry(scan, where, rounds):
    return dict(kind=JPEG_PROG_KINDS[scan.kind], components=tuple(scan.comp[:scan.ncomp]), band=(scan.ss, scan.se), ah=scan.ah, al=scan.al,
                bytes=scan.end - scan.begin, decoded=where, sync_rounds=rounds)


def jpeg_prog_entropy_device(host, ops, device, subsequence_bits, max_sync_rounds, timing=None):
    """the scans of a JpegProgHost in file order on one stream -> (status, per-scan entries, coefficients int16 [nblocks,64] on the device,
    bytes uploaded, bytes downloaded).  DC-first, AC-first and DC-refinement scans are decoded on the device; an AC-refinement scan on the
    host against the component's non-zero masks (downloaded once per component, again only if an AC-first scan of it ran since) and its
    records are applied on the device.  status JPEG_NOT_CONVERGED: a scan exceeded max_sync_rounds, nothing usable in the coefficients.
    timing: a dict that receives the seconds spent in 'device_scans' (with their host preparation and uploads), 'mask_download',
    'host_refine' (with the scan's preparation), 'record_upload' and 'apply'; each part then ends in a synchronise, which the untimed
    path does not do."""
    import time
    h = host.header
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt)).to(device)           # noqa: E731
    coef = torch.zeros((h.nblocks, 64), dtype=torch.int16, device=device)
    maps, masks, entries, uploaded, downloaded = {}, {}, [], 0, 0

    def sync():
        if timing is not None and device.type == "cuda":
            torch.cuda.synchronize(device)

    def tick(key, t0):
        if timing is not None:
            sync()
            timing[key] = timing.get(key, 0.0) + time.perf_counter() - t0

    def block_map(scan):
        nonlocal uploaded
        if scan.ncomp > 1:
            return None
        c = scan.comp[0]
        if c not in maps:
            m = host.block_map(scan)
            maps[c] = up(m, np.int32)
            uploaded += m.nbytes
        return maps[c]

    for scan in host.scans:
        sync()
        t0 = time.perf_counter()
        data, segs = host.prepare(scan)
        bmap = block_map(scan)
        kind = JPEG_PROG_KINDS[scan.kind]
        if kind in ("dc_first", "ac_first"):
            lanes, segx, longest = host.plan(scan, segs, subsequence_bits)
            tables = host.tables(scan)
            ws = torch.empty(ops.jpeg_prog_workspace(lanes.shape[0], scan.nblocks), dtype=torch.uint8, device=device)
            rc, rounds = ops.jpeg_prog_decode_scan(h, scan, up(data, np.uint8), up(lanes, np.int32), up(segx, np.int32), longest,
                                                   up(tables, np.int32), bmap, max_sync_rounds, ws, coef)
            uploaded += data.nbytes + lanes.nbytes + segx.nbytes + tables.nbytes
            if rc == JPEG_NOT_CONVERGED:
                return rc, entries, coef, uploaded, downloaded
            _jpeg_check(rc, "pf_jpeg_prog_decode_scan")
            if kind == "ac_first" and scan.comp[0] in masks:
                masks[scan.comp[0]] = None                       # the component's non-zero map changed on the device
            entries.append(_scan_entry(scan, "device", rounds))
            tick("device_scans", t0)
        elif kind == "dc_refine":
            ops.jpeg_prog_dc_refine(h, scan, up(data, np.uint8), up(segs, np.int32), bmap, coef)
            uploaded += data.nbytes + segs.nbytes
            entries.append(_scan_entry(scan, "device", 0))
            tick("device_scans", t0)
        else:
            c = scan.comp[0]
            tick("host_refine", t0)
            if masks.get(c) is None:
                t0 = time.perf_counter()
                m = ops.jpeg_prog_nonzero_mask(h, scan, coef, bmap, torch.empty(scan.nblocks, dtype=torch.int64, device=device))
                masks[c] = np.ascontiguousarray(m.cpu().numpy()).view(np.uint64)
                downloaded += masks[c].nbytes
                tick("mask_download", t0)
            t0 = time.perf_counter()
            rec = host.refine_ac(scan, masks[c], (data, segs))
            tick("host_refine", t0)
            t0 = time.perf_counter()
            records = up(rec, np.int64)
            uploaded += rec.nbytes
            tick("record_upload", t0)
            t0 = time.perf_counter()
            ops.jpeg_prog_apply_refinement(h, scan, records, bmap, coef)
            tick("apply", t0)
            entries.append(_scan_entry(scan, "host", 0))
    return 0, entries, coef, uploaded, downloaded


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


def decode_jpeg(data, device="cuda", entropy="device", apply_orientation=True, subsequence_bits=None, max_sync_rounds=None, ops=None,
                progressive=False):
    """Baseline JPEG (bytes or a path) -> (uint8 [H,W,3] RGB device tensor, JpegInfo), bit-exact with libjpeg's defaults (islow, fancy
    upsampling): what ``cv2.imread`` + BGR->RGB gives (apply_orientation=True) or PIL (False).  entropy='device' uploads the compressed
    scan and decodes it in subsequences on the GPU; 'host' runs the sequential C decoder and uploads the coefficients.
    When the device path needs more than max_sync_rounds rounds the entropy step completes on the host path (info.entropy says so); the
    pixels are the same either way.  Unsupported files raise a JpegError subclass (a ValueError); there is no fallback to a host library.
    progressive=True also accepts progressive files (SOF2) with a complete progression, again bit-exact with libjpeg; a baseline file
    takes the baseline path unchanged.  entropy='device' then decodes the DC-first, AC-first and DC-refinement scans on the GPU and the
    AC-refinement scans on the host (info.scans says where each scan went); 'host' runs the sequential decoder over every scan.  A scan
    that exceeds max_sync_rounds completes the whole file on the host path."""
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
    if progressive:
        prog = JpegProgHost(data)
        if not prog.baseline:
            return _decode_jpeg_progressive(prog, ops, dev, entropy, apply_orientation, S, cap)
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
                    orientation=h.orientation, entropy=used, sync_rounds=rounds, subsequence_bits=S, bytes_uploaded=uploaded,
                    progressive=False, scans=[])
    return rgb, info


def _decode_jpeg_progressive(host, ops, dev, entropy, apply_orientation, S, cap):
    """decode_jpeg for a progressive file (a JpegProgHost that is not baseline)"""
    h = host.header
    used, uploaded, downloaded, coef, scans = entropy, 0, 0, None, None
    if entropy == "device":
        rc, scans, coef, uploaded, downloaded = jpeg_prog_entropy_device(host, ops, dev, S, cap)
        if rc == JPEG_NOT_CONVERGED:
            used = "host"                        # round cap exceeded in some scan: the whole file from the sequential decoder
    if used == "host":
        c = host.decode_entropy()
        uploaded += c.nbytes
        coef = torch.from_numpy(c).to(dev)
        scans = [_scan_entry(s, "host", 0) for s in host.scans]
    o = h.orientation if apply_orientation else 1
    H, W = (h.width, h.height) if o >= 5 else (h.height, h.width)
    rgb = torch.empty((H, W, 3), dtype=torch.uint8, device=dev)
    ops.jpeg_reconstruct(h, coef, o, torch.empty(ops.jpeg_workspace(h, 0)[1], dtype=torch.uint8, device=dev), rgb)
    info = JpegInfo(width=h.width, height=h.height, components=h.ncomp, sampling=(h.hmax, h.vmax),
                    restart_interval=max(s.restart_interval for s in host.scans), orientation=h.orientation, entropy=used,
                    sync_rounds=max(e["sync_rounds"] for e in scans), subsequence_bits=S, bytes_uploaded=uploaded,
                    bytes_downloaded=downloaded, progressive=True, scans=scans)
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
