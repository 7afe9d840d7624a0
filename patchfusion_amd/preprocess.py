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


# ---------------------------------------------------------------- PNG
# Defaults of decode_png.  A zlib block holds at most 32 767 symbols of at most 48 bits (15 + 5 + 15 + 13) behind about 4.5 kbit of
# header: under 1.6 Mbit, so 2^21 bits bound every block zlib writes.  zlib chooses a fixed block only where it is smaller than a dynamic
# one (typically the last), and each one the walk meets costs one more scan pass: 8 passes.
# The inflate arm was chosen by tools/png_decode_time.py (profiles/png_decode_time.json, one MI355X).  The device arm decodes a block
# sequentially on one wave, twice (scan and inflate passes), so those two passes take about 14 ms (PIL level 6) to 27 ms (level 1)
# whatever the file's size: at 3840x2160 that beats the host arm (RGB8 level 6: 32.6 ms against 76.2 ms, and 93.4 ms for PIL + upload),
# at 2048x1024 it does not (18.8 ms against 16.9 ms; level 1: 32.1 against 22.4).  The rule was "default only if faster at both sizes",
# so 'host' is the default and 'device' is opt-in.
PNG_MAX_BLOCK_BITS = 1 << 21
PNG_MAX_CHAIN_ROUNDS = 8
PNG_INFLATE = "host"
# block_decode='subsequences' (opt-in, csrc/png_inflate_par.hip): a block goes to one workgroup of PNG_PAR_WINDOW threads and every thread
# decodes one lane of subsequence_bits bits of it.  PNG_PAR_WINDOW restates PF_PNGD_PAR_WINDOW of csrc/png_inflate.h (the library
# answers pf_pngd_par_window()).  Both numbers were chosen by tools/png_decode_time.py --subsequences (profiles/png_inflate_par_time.json,
# one MI355X) with the rule "lowest sum of the whole-decode medians on the two RGB level-6 files (2048x1024 + 3840x2160)".  Workgroup
# size at 256-bit lanes: 1024 threads 4.93 + 16.68 = 21.61 ms, 512 threads 5.11 + 16.35 = 21.46 ms, 256 threads 5.26 + 16.26 = 21.52 ms
# (1024 is faster at the small file and slower at the large one, whose 759 workgroups then do not fit the device at once).  Lane length
# at 512 threads: 128 bits 21.46 ms, 256 bits 21.46 ms, 512 bits 21.44 ms, 1024 bits 22.03 ms: the first three are level inside the
# min-max spread (0.1 - 0.5 ms), and 256 is also level with the best on the other six files of the table, where 128 loses up to 0.9 ms
# (level-1 files, 12 - 17 rounds).  The mode's scan + inflate stages take 0.8 and 1.1 ms against the sequential arm's 14.4 and 15.5 ms,
# and the whole decode beats inflate='host' at both sizes (5.1 against 16.8 ms, 16.4 against 76.8 ms); the defaults above are left as
# they are on purpose.
PNG_BLOCK_DECODE = "sequential"
PNG_SUBSEQUENCE_BITS = 256
PNG_PAR_WINDOW = 512
PNG_S_OK, PNG_S_INVALID, PNG_S_LIMIT, PNG_S_EOS, PNG_S_SIZE, PNG_S_DIST = range(6)       # PF_PNGD_S_* of pf_hip.h
PNG_F_STREAM, PNG_F_DISTANCE, PNG_F_FILTER, PNG_F_PLTE = 1, 2, 4, 8                    # PF_PNGD_F_*
PNG_PAD_WORDS = 2                                                                      # PF_PNGD_PAD_WORDS


class PngError(ValueError):
    """a PNG file decode_png refuses or cannot decode; .code is the PF_PNGD_E_* status of include/pf_hip.h"""

    def __init__(self, code, what):
        super().__init__(f"png: {what}")
        self.code = code


def _png_refusal(name, what):
    return type(name, (PngError,), {"__doc__": what})


PNG_ERRORS = {
    80: _png_refusal("PngSignature", "not a PNG file (bad signature)"),
    81: _png_refusal("PngChunk", "a chunk's length runs past the file, a critical chunk is unknown, or tRNS does not fit the colour type"),
    82: _png_refusal("PngOrder", "chunks out of order (IHDR first, PLTE before IDAT, IDAT consecutive, IEND last)"),
    83: _png_refusal("PngCrc", "CRC mismatch in a critical chunk"),
    84: _png_refusal("PngIhdr", "IHDR holds a combination the specification forbids"),
    85: _png_refusal("PngInterlaced", "Adam7 interlaced files are not supported"),
    86: _png_refusal("PngZlibHeader", "zlib header: method other than deflate, window above 32 KiB, preset dictionary, or bad check bits"),
    87: _png_refusal("PngStream", "the deflate stream is invalid or truncated"),
    88: _png_refusal("PngDistance", "a match reaches before the start of the output"),
    89: _png_refusal("PngSize", "the inflated size is not height * (1 + row bytes)"),
    90: _png_refusal("PngAdler", "Adler-32 mismatch"),
    91: _png_refusal("PngFilter", "a row's filter type is above 4"),
    92: _png_refusal("PngPalette", "PLTE is missing or invalid, or a pixel indexes past it"),
    93: _png_refusal("PngIdatCrc", "CRC mismatch in an IDAT chunk"),
}
PngInterlaced = PNG_ERRORS[85]


def _png_raise(code):
    cls = PNG_ERRORS[code]
    raise cls(code, cls.__doc__)


def _png_check(rc, step):
    if rc == 0:
        return
    if rc in PNG_ERRORS:
        _png_raise(rc)
    raise PngError(rc, f"{step} failed (status {rc})")


class PngInfo:
    """what decode_png reports next to the image"""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def __repr__(self):
        return "PngInfo(" + ", ".join(f"{k}={v!r}" for k, v in self.__dict__.items()) + ")"


class PngHost:
    """the HOST ONLY steps of the PNG decoder (csrc/png_host.h through the C ABI, and the chain walk): no GPU call"""

    def __init__(self, data, check_idat_crc=False):
        self.lib = _lib.load()
        self.data = np.frombuffer(bytes(data), dtype=np.uint8)
        self.header = _lib.PngdHeader()
        buf = np.zeros(self.data.size + 16, dtype=np.uint8)
        n = C.c_long()
        _png_check(self.lib.pf_pngd_parse(self.data.ctypes.data, self.data.size, int(bool(check_idat_crc)), C.byref(self.header), buf.ctypes.data,
                                          self.data.size, C.byref(n)), "pf_pngd_parse")
        self.deflate = buf[:n.value]                 # raw deflate data and the Adler-32 behind it (the zlib header is checked and gone)

    def words(self):
        """the deflate bytes as the device wants them: little-endian words with PNG_PAD_WORDS zero words behind"""
        n = self.deflate.size
        w = np.zeros(4 * ((n + 3) // 4 + PNG_PAD_WORDS), dtype=np.uint8)
        w[:n] = self.deflate
        return w.view(np.int32)

    def bits(self, p, k):
        """k <= 16 bits at bit p of the deflate data, first bit lowest (zeros past the end)"""
        d, i = self.deflate, p >> 3
        v = sum(int(d[i + j]) << (8 * j) for j in range(3) if i + j < d.size)
        return (v >> (p & 7)) & ((1 << k) - 1)

    def inflate(self):
        """stdlib zlib over the raw deflate data -> (the inflated bytes, the Adler-32 the file states)"""
        import zlib
        expected = self.header.inflated_bytes
        z = zlib.decompressobj(wbits=-15)
        try:
            out = z.decompress(self.deflate.tobytes(), expected + 1)
        except zlib.error as e:
            _png_raise(88 if "distance too far back" in str(e) else 87)
        if len(out) > expected or (z.eof and len(out) != expected):
            _png_raise(89)
        if not z.eof or len(z.unused_data) < 4:
            _png_raise(87)
        return np.frombuffer(bytearray(out), dtype=np.uint8), int.from_bytes(z.unused_data[:4], "big")


class PngChain:
    """The chain walk over the scan records: from bit 0, a scanned block jumps to its recorded end, a stored block is closed-form from the
    host's bytes.  step() -> None when the final block was reached (blocks, adler and counts are set), or the start bit of a fixed block
    that has no record yet (add() its record and call step() again).  A stream that cannot be right raises; .giveup names what only the
    host arm can complete."""

    def __init__(self, host):
        self.host, self.table, self.blocks, self.p, self.total, self.giveup = host, {}, [], 0, 0, None
        self.counts = {"dynamic": 0, "fixed": 0, "stored": 0}

    def add(self, records):
        for start, end, out, st in np.asarray(records, dtype=np.int64).reshape(-1, 4):
            self.table[int(start) & 0xffffffff] = (int(end) & 0xffffffff, int(out) & 0xffffffff, int(st) & 255)

    def step(self):
        host = self.host
        d, nbits, expected = host.deflate, 8 * host.deflate.size, host.header.inflated_bytes
        while True:
            p = self.p
            if p + 3 > nbits:
                _png_raise(87)
            head = host.bits(p, 3)
            kind = head >> 1
            if kind == 3:
                _png_raise(87)
            if kind == 0:
                at = (p + 3 + 7) // 8
                if at + 4 > d.size:
                    _png_raise(87)
                n, inv = int(d[at]) | int(d[at + 1]) << 8, int(d[at + 2]) | int(d[at + 3]) << 8
                if n ^ inv != 0xffff or at + 4 + n > d.size:
                    _png_raise(87)
                self.blocks.append((at + 4, 0, self.total, n))
                self.p, out = 8 * (at + 4 + n), n
            else:
                rec = self.table.get(p)
                if rec is None:
                    if kind == 1:
                        return p
                    _png_raise(87)                   # a dynamic header the finder's test refuses is not a header
                end, out, st = rec
                if st == PNG_S_LIMIT:
                    self.giveup = "a block is longer than max_block_bits"
                    return None
                if st != PNG_S_OK:
                    _png_raise(89 if st == PNG_S_SIZE else 87)
                self.blocks.append((p, kind, self.total, out))
                self.p = end
            self.counts[("stored", "fixed", "dynamic")[kind]] += 1
            self.total += out
            if self.total > expected:
                _png_raise(89)
            if head & 1:
                break
        if self.total != expected:
            _png_raise(89)
        at = (self.p + 7) // 8
        if at + 4 > d.size:
            _png_raise(87)
        self.adler = int.from_bytes(d[at:at + 4].tobytes(), "big")
        return None


def _png_subsequence_bits(value):
    bits = PNG_SUBSEQUENCE_BITS if value is None else value
    if isinstance(bits, bool) or not isinstance(bits, (int, np.integer)) or bits < 64 or bits > (1 << 16) or bits % 32:
        raise ValueError(f"subsequence_bits must be a multiple of 32 in 64 .. 2^16, got {value!r}")
    return int(bits)


def png_inflate_device(host, ops, dev, max_chain_rounds, max_block_bits, timing=None, block_decode="sequential", subsequence_bits=None):
    """the device inflate of decode_png on a PngHost -> (inflated uint8 [height * (1 + rowbytes)] on the device or None, stats).  None:
    stats['fallback_reason'] says what only the host arm can complete; nothing was decoded.  The stream's own errors raise.
    timing: a dict that receives the seconds of 'finder', 'scan', 'chain_walk' (with its copies), 'inflate' and 'resolve'; each part then
    ends in a synchronise, which the untimed path does not do.
    block_decode='subsequences' runs the scan and inflate passes of csrc/png_inflate_par.hip with lanes of subsequence_bits bits; the
    stats then carry 'sync_rounds' as a device word until decode_png reads it back with the status."""
    import time
    if block_decode not in ("sequential", "subsequences"):
        raise ValueError(f"block_decode must be 'sequential' or 'subsequences', got {block_decode!r}")
    par = block_decode == "subsequences"
    S = _png_subsequence_bits(subsequence_bits) if par else None
    h = host.header
    n, expected = host.deflate.size, h.inflated_bytes
    stats = dict(candidates=0, chain_rounds=0, resolve_rounds=0, blocks=None, bytes_uploaded=0, bytes_downloaded=0, fallback_reason=None, adler=None)
    t0 = time.perf_counter()

    def tick(key):
        nonlocal t0
        if timing is not None:
            if dev.type == "cuda":
                torch.cuda.synchronize(dev)
            now = time.perf_counter()
            timing[key] = timing.get(key, 0.0) + now - t0
            t0 = now

    def give_up(why):
        stats["fallback_reason"] = why
        return None, stats

    if n == 0:
        _png_raise(87)
    if n >= (1 << 28) or expected >= (1 << 31):
        return give_up("the stream is too large for 32-bit positions")
    if max_chain_rounds < 1:
        return give_up("max_chain_rounds allows no scan pass")
    nbits = 8 * n
    w = host.words()
    words = torch.from_numpy(w).to(dev)
    stats["bytes_uploaded"] += w.nbytes
    cand = torch.empty(n // 16 + 64, dtype=torch.int32, device=dev)
    count = torch.zeros(1, dtype=torch.int32, device=dev)
    ops.pngd_find(words, nbits, cand, count)
    ncand = int(count.cpu()[0])
    stats["bytes_downloaded"] += 4
    stats["candidates"] = ncand
    tick("finder")
    if ncand > cand.numel():
        return give_up("the candidate list overflowed")
    chain = PngChain(host)
    starts, nstart = cand, ncand
    if par:
        stats["sync_rounds"] = torch.zeros(1, dtype=torch.int32, device=dev)
    while True:
        stats["chain_rounds"] += 1
        if nstart:
            records = torch.empty((nstart, 4), dtype=torch.int32, device=dev)
            if par:
                ops.pngd_scan_par(words, nbits, starts, nstart, max_block_bits, min(expected, 0xffffffff), S, records, stats["sync_rounds"])
            else:
                ops.pngd_scan(words, nbits, starts, nstart, max_block_bits, min(expected, 0xffffffff), records)
            tick("scan")
            chain.add(records.cpu().numpy())
            stats["bytes_downloaded"] += 16 * nstart
        need = chain.step()
        if need is None:
            break
        if stats["chain_rounds"] >= max_chain_rounds:
            tick("chain_walk")
            return give_up("more fixed blocks than max_chain_rounds scan passes reach")
        starts, nstart = torch.tensor([need], dtype=torch.int64).to(torch.int32).to(dev), 1
        stats["bytes_uploaded"] += 4
        tick("chain_walk")
    if chain.giveup:
        tick("chain_walk")
        return give_up(chain.giveup)
    table = np.asarray(chain.blocks, dtype=np.int64).astype(np.uint32).view(np.int32).reshape(-1, 4)
    blocks = torch.from_numpy(table).to(dev)
    stats["bytes_uploaded"] += table.nbytes
    tick("chain_walk")
    stats["blocks"], stats["adler"] = dict(chain.counts), chain.adler
    lit = torch.empty(expected, dtype=torch.uint8, device=dev)
    ref = torch.empty(expected, dtype=torch.int32, device=dev)
    stats["status"] = torch.zeros(1, dtype=torch.int32, device=dev)
    units = len(chain.blocks)
    if par:
        ops.pngd_inflate_par(words, nbits, blocks, expected, S, lit, ref, stats["status"], stats["sync_rounds"])
        # a reference now points into an earlier lane's range: the lanes a block's bits touch (from its header on, so never too few)
        units = sum(1 if kind == 0 else (chain.table[p][0] + S - 1) // S - p // S for p, kind, _, _ in chain.blocks)
    else:
        ops.pngd_inflate(words, nbits, blocks, expected, lit, ref, stats["status"])
    tick("inflate")
    stats["resolve_rounds"] = max(units - 1, 0).bit_length() + 1                      # ceil(log2(blocks or lane ranges)) + 1
    inflated = ops.pngd_resolve(lit, ref, stats["resolve_rounds"], torch.empty(expected, dtype=torch.uint8, device=dev))
    tick("resolve")
    return inflated, stats


def decode_png(data, device="cuda", inflate=None, verify=True, max_chain_rounds=None, max_block_bits=None, ops=None, timing=None,
               block_decode=None, subsequence_bits=None):
    """PNG (bytes or a path) -> (device tensor, PngInfo), lossless and bit-exact with the PNG specification: uint8 or torch.uint16 (native
    byte order), [H,W] for grey, [H,W,2] grey+alpha, [H,W,3] RGB, [H,W,4] RGBA.  A palette expands to uint8 [H,W,3] (tRNS is ignored and
    reported as info.has_trns); grey of 1 / 2 / 4 bits expands to uint8 by bit replication (x255, x85, x17) as libpng's
    expand_gray_1_2_4_to_8, PIL and cv2 do.  Every non-interlaced colour type and bit depth is accepted; ancillary chunks are skipped.
    inflate='device' uploads the compressed stream and inflates it block-parallel on the GPU; 'host' runs the standard library's zlib and
    uploads the filtered bytes; unfilter, expansion and the Adler-32 are the same device code either way, and so are the pixels.  When the
    device arm gives up (candidate list overflow, a block above max_block_bits, more fixed blocks than max_chain_rounds scan passes) the
    host arm completes the file: info.inflate and info.fallback_reason say so.  block_decode='subsequences' (with inflate='device'
    only) decodes inside a block in parallel, every thread of a workgroup one lane of subsequence_bits bits (a multiple of 32 in
    64 .. 2^16, default PNG_SUBSEQUENCE_BITS); info.sync_rounds is the largest number of rounds a window of lanes needed to agree
    (0 for 'sequential').  verify=True checks the Adler-32 (computed on the device),
    verify='full' also the CRC-32 of the IDAT chunks (on the host: one more pass over the compressed bytes), verify=False neither.
    Unsupported or broken files raise a PngError subclass (a ValueError); there is no fallback to a host image library."""
    inflate = PNG_INFLATE if inflate is None else inflate
    if inflate not in ("device", "host"):
        raise ValueError(f"inflate must be 'device' or 'host', got {inflate!r}")
    if verify not in (True, False, "full"):
        raise ValueError(f"verify must be True, False or 'full', got {verify!r}")
    block_decode = PNG_BLOCK_DECODE if block_decode is None else block_decode
    if block_decode not in ("sequential", "subsequences"):
        raise ValueError(f"block_decode must be 'sequential' or 'subsequences', got {block_decode!r}")
    if block_decode == "subsequences" and inflate != "device":
        raise ValueError("block_decode='subsequences' needs inflate='device'")
    lane_bits = _png_subsequence_bits(subsequence_bits)
    rounds_cap = PNG_MAX_CHAIN_ROUNDS if max_chain_rounds is None else int(max_chain_rounds)
    bits_cap = PNG_MAX_BLOCK_BITS if max_block_bits is None else int(max_block_bits)
    if rounds_cap < 0:
        raise ValueError("max_chain_rounds must be >= 0")
    if bits_cap < 64 or bits_cap > (1 << 31):
        raise ValueError(f"max_block_bits must be in 64 .. 2^31, got {max_block_bits}")
    if isinstance(data, (str, os.PathLike)):
        with open(data, "rb") as f:
            data = f.read()
    if not isinstance(data, (bytes, bytearray, memoryview)):
        raise ValueError(f"decode_png expects bytes or a path, got {type(data).__name__}")
    if ops is None:
        from .hip_ops import ops as _ops        # fails loudly when the HIP extension is missing
        ops = _ops
    import time
    dev = torch.device(device)
    host = PngHost(data, check_idat_crc=verify == "full")
    h = host.header
    expected = h.inflated_bytes
    if expected >= (1 << 31):
        raise PngError(89, "images above 2 GiB of filtered bytes are not supported")
    used, inflated, stated = inflate, None, None
    stats = dict(candidates=0, chain_rounds=0, resolve_rounds=0, blocks=None, bytes_uploaded=0, bytes_downloaded=0, fallback_reason=None)
    if inflate == "device":
        inflated, stats = png_inflate_device(host, ops, dev, rounds_cap, bits_cap, timing, block_decode, lane_bits)
        stated = stats.get("adler")
        if inflated is None:
            used = "host"
            stats.pop("sync_rounds", None)
    if used == "host":
        t0 = time.perf_counter()
        raw, stated = host.inflate()
        inflated = torch.from_numpy(raw).to(dev)
        stats["bytes_uploaded"] += raw.nbytes
        if timing is not None:
            timing["host_inflate"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    # {Adler-32, status flags} and, behind a subsequence decode, its sync rounds: the one 8- or 12-byte copy back
    result = torch.zeros(3 if "sync_rounds" in stats else 2, dtype=torch.int32, device=dev)
    status = result[1:2]
    if "status" in stats:
        status.copy_(stats.pop("status"))
    if "sync_rounds" in stats:
        result[2:].copy_(stats.pop("sync_rounds"))
    if verify:
        ops.pngd_adler(inflated, torch.empty(2, dtype=torch.int64, device=dev), result)
        if timing is not None and dev.type == "cuda":
            torch.cuda.synchronize(dev)
            timing["adler"] = time.perf_counter() - t0
            t0 = time.perf_counter()
    H, W, ch = h.height, h.width, 3 if h.color_type == 3 else h.channels
    shape = (H, W) if ch == 1 else (H, W, ch)
    image = torch.empty(shape, dtype=torch.uint16 if h.depth == 16 else torch.uint8, device=dev)
    if h.depth == 8 and h.color_type != 3:
        ops.pngd_unfilter(h, inflated, image, status)                   # the unfiltered rows are the image
    else:
        recon = ops.pngd_unfilter(h, inflated, torch.empty(H * h.rowbytes, dtype=torch.uint8, device=dev), status)
        palette = None
        if h.color_type == 3:
            palette = torch.from_numpy(np.frombuffer(bytes(h.palette), dtype=np.uint8).copy()).to(dev)
            stats["bytes_uploaded"] += 768
        ops.pngd_expand(h, recon, palette, image, status)
    got = result.cpu().numpy().view(np.uint32)
    stats["bytes_downloaded"] += 4 * got.size
    if timing is not None:
        timing["unfilter_expand"] = time.perf_counter() - t0
    flags = int(got[1])
    for bit, code in ((PNG_F_DISTANCE, 88), (PNG_F_STREAM, 87), (PNG_F_FILTER, 91), (PNG_F_PLTE, 92)):
        if flags & bit:
            _png_raise(code)
    if verify and int(got[0]) != stated:
        _png_raise(90)
    info = PngInfo(width=W, height=H, bit_depth=h.depth, color_type=h.color_type, channels=h.channels, has_trns=bool(h.has_trns),
                   inflate=used, fallback_reason=stats["fallback_reason"], blocks=stats["blocks"], candidates=stats["candidates"],
                   chain_rounds=stats["chain_rounds"], resolve_rounds=stats["resolve_rounds"], compressed_bytes=int(h.compressed_bytes),
                   bytes_uploaded=stats["bytes_uploaded"], bytes_downloaded=stats["bytes_downloaded"],
                   block_decode=block_decode if used == "device" else "sequential", subsequence_bits=lane_bits,
                   sync_rounds=int(got[2]) if got.size > 2 else 0)
    return image, info


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

    def read(self, path_or_bytes, png_options=None, **kw):
        """decode_jpeg or decode_png (by the file's signature) followed by __call__: the file never becomes a host array.
        JPEG: the EXIF orientation is applied for the datasets the reference reads with cv2.imread ('mid', general) and not for
        'cityscapes', which it reads with PIL (no rotation); kw goes to decode_jpeg.  PNG: decode_png(**png_options), then one kernel to
        uint8 [H,W,3]: grey replicated, alpha dropped, 16-bit samples keep their high byte (libpng's strip_16, what cv2.imread and, for
        16-bit RGB, PIL do); kw (JPEG-only keywords) is ignored.  'u4k' files are raw arrays, not JPEG: refused."""
        if self.dataset_name == "u4k":
            raise ValueError("dataset 'u4k' stores raw arrays, not JPEG files: there is nothing to decode")
        if isinstance(path_or_bytes, (str, os.PathLike)):
            with open(path_or_bytes, "rb") as f:
                path_or_bytes = f.read()
        if isinstance(path_or_bytes, (bytes, bytearray, memoryview)) and bytes(path_or_bytes[:8]) == b"\x89PNG\r\n\x1a\n":
            image, self.last_png_info = decode_png(path_or_bytes, device=self.device, ops=self.ops, **(png_options or {}))
            if image.dtype != torch.uint8 or image.dim() != 3 or image.shape[2] != 3:
                image = self.ops.pngd_to_rgb8(image, torch.empty(tuple(image.shape[:2]) + (3,), dtype=torch.uint8, device=self.device))
            return self(image)
        kw.setdefault("apply_orientation", self.dataset_name != "cityscapes")
        rgb, self.last_jpeg_info = decode_jpeg(path_or_bytes, device=self.device, ops=self.ops, **kw)
        return self(rgb)
