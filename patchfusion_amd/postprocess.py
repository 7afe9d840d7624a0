"""Device-side output stage: what ``Tester.run`` (estimator/tester/tester.py:66-84) does on the
CPU with the stitched depth map - colour rendering, 16-bit export, evaluation metrics - as HIP kernels on the
depth tensor where it already lives.  Same names and arguments as the reference functions; results come back as
small device tensors / python floats (one 104-byte D2H for the metrics).  There is no CPU path.
"""
import math
import os
import struct
import zlib

import numpy as np
import torch

_LUTS = {}


def _ops():
    from .hip_ops import ops        # fails loudly when the HIP extension is missing
    return ops


def _plane_any(value):
    """squeeze to one [H,W] plane, dtype kept (masks)"""
    v = value.detach()
    while v.dim() > 2 and v.shape[0] == 1:
        v = v[0]
    if v.dim() != 2:
        raise ValueError(f"expected one map, got shape {tuple(value.shape)}")
    return v


def colormap_lut(cmap, device):
    """(N+3, 4) uint8 table of a matplotlib colormap (N colours + under / over / bad rows), scaled like
    Colormap.__call__(bytes=True); built once per (cmap, device) on the host - it is 1 KiB of constants."""
    key = (cmap, str(device))
    if key not in _LUTS:
        import matplotlib
        cm = matplotlib.colormaps[cmap] if hasattr(matplotlib, "colormaps") else matplotlib.cm.get_cmap(cmap)
        if not cm._isinit:
            cm._init()
        _LUTS[key] = (torch.from_numpy((cm._lut * 255).astype(np.uint8)).to(device).contiguous(), int(cm.N))
    return _LUTS[key]


def _plane(value):
    v = value.detach()
    while v.dim() > 2 and v.shape[0] == 1:
        v = v[0]
    if v.dim() != 2:
        raise ValueError(f"expected one depth map, got shape {tuple(value.shape)}")
    return v.float().contiguous()


def gamma_table():
    """color.py:86-91 on one byte: (img / 255) ** 2.2 * 255 in float64, truncated by astype(uint8)."""
    return (np.power(np.arange(256) / 255, 2.2) * 255).astype(np.uint8)


def _invalid_mask_u8(invalid_mask, d):
    if invalid_mask is None:
        return None
    m = torch.as_tensor(np.asarray(invalid_mask.detach().cpu()) if isinstance(invalid_mask, torch.Tensor) else np.asarray(invalid_mask))
    return (m.reshape(d.shape) != 0).to(torch.uint8).to(d.device).contiguous()


def _range(d, vmin, vmax, q0, q1, invalid_val, m, ops):
    """device float32 [2] = (vmin, vmax); a None end is the q0 / q1 percentile of the pixels that invalid_val / m leave"""
    if vmin is None or vmax is None:
        vmm = ops.percentiles(d, q0, q1, invalid_val=invalid_val, invalid_mask=m)
        if vmin is not None:
            vmm[0] = float(vmin)
        if vmax is not None:
            vmm[1] = float(vmax)
        return vmm
    return torch.tensor([float(vmin), float(vmax)], dtype=torch.float32).to(d.device)


_LAYOUTS = {"rgba": (0, 4), "bgr": (1, 3)}


def _render(d, m, vmm, cmap, invalid_val, background_color, gamma_corrected, value_transform, layout, ops):
    """normalised colour lookup of plane d with range vmm -> uint8 [H,W,4] ('rgba') or [H,W,3] ('bgr')"""
    if layout not in _LAYOUTS:
        raise ValueError(f"layout {layout!r}: expected 'rgba' or 'bgr'")
    lut, N = colormap_lut(cmap, d.device)
    bg = tuple(int(v) & 255 for v in background_color)
    if gamma_corrected:
        g = gamma_table()
        lut = torch.from_numpy(g[lut.cpu().numpy()]).to(d.device).contiguous()
        bg = tuple(int(g[v]) for v in bg)
    code, ch = _LAYOUTS[layout]
    out = torch.empty(d.shape + (ch,), dtype=torch.uint8, device=d.device)
    if value_transform is not None:
        if m is None:
            m = (d == invalid_val).to(torch.uint8) if invalid_val is not None else torch.zeros_like(d, dtype=torch.uint8)
        lo, hi = (np.float32(t) for t in vmm.tolist())
        x = d.cpu().numpy()
        x = (x - lo) / (hi - lo) if lo != hi else x * np.float32(0)
        x[m.cpu().numpy() != 0] = np.nan
        x = np.ascontiguousarray(np.asarray(value_transform(x), dtype=np.float32))
        d = torch.from_numpy(x).to(d.device)
        vmm = torch.tensor([0.0, 1.0], dtype=torch.float32).to(d.device)        # (x - 0) / (1 - 0) == x exactly
    if code == 0:
        return ops.colorize(d, vmm, lut, N, invalid_val, bg, out, invalid_mask=m)
    return ops.colorize_ex(d, vmm, lut, N, invalid_val, bg, out, invalid_mask=m, layout=code)


def colorize(value, vmin=None, vmax=None, cmap="turbo_r", invalid_val=-99, invalid_mask=None, background_color=(128, 128, 128, 255),
             gamma_corrected=False, value_transform=None, vminp=2, vmaxp=95, ops=None, layout="rgba"):
    """estimator/utils/color.py:95-150 on the device: -> uint8 tensor [H,W,4] (RGBA).  vmin / vmax default to the
    exact 2nd / 95th percentile of the valid pixels (radix select, no sort, no host round trip).

    invalid_mask (bool, same grid; numpy or tensor) replaces the `value == invalid_val` test as in the reference (:121-122).
    gamma_corrected is a per-byte function (:86-91), so it is applied to the 1 KiB colour table and the background colour, not to the
    image.  value_transform is an arbitrary python callable on the normalised numpy array (:140-141): only in that case the
    normalised plane makes one host round trip (the reference hands the callable a numpy array with NaN at the invalid pixels).
    layout='bgr' writes uint8 [H,W,3] = `colorize(...)[:, :, [2, 1, 0]]` (tester.py:69-71, the array cv2.imwrite takes) directly."""
    ops = ops or _ops()
    d = _plane(value)
    m = _invalid_mask_u8(invalid_mask, d)
    vmm = _range(d, vmin, vmax, vminp, vmaxp, invalid_val, m, ops)
    return _render(d, m, vmm, cmap, invalid_val, background_color, gamma_corrected, value_transform, layout, ops)


def colorize_infer_pfv1(value, cmap="magma_r", vmin=None, vmax=None, ops=None):
    """estimator/utils/color.py:8-25 on the device: -> uint8 tensor [H,W,3] in B, G, R order.  vmin defaults to the minimum and vmax to
    the 95th percentile of ALL values (no invalid handling, :10-12); vmin == vmax maps every pixel to 0 (:16-17)."""
    ops = ops or _ops()
    d = _plane(value)
    vmm = _range(d, vmin, vmax, 0, 95, None, None, ops)
    return _render(d, None, vmm, cmap, None, (0, 0, 0, 0), False, None, "bgr", ops)


def colorize_rescale(value, vmin=None, vmax=None, cmap="turbo_r", invalid_val=-99, invalid_mask=None, background_color=(128, 128, 128, 255),
                     gamma_corrected=False, value_transform=None, vminp=2, vmaxp=95, ops=None):
    """estimator/utils/color.py:28-93 on the device: -> uint8 tensor [H,W,4] (RGBA).  colorize with another range: vmin / vmax default
    to the minimum / maximum over ALL values, invalid ones included (:63-64) -- what the reference computes, kept.  Invalid pixels
    still go through the colormap's "bad" colour and end as background_color (:75,:84); vminp / vmaxp are accepted and unused as there."""
    ops = ops or _ops()
    d = _plane(value)
    m = _invalid_mask_u8(invalid_mask, d)
    vmm = _range(d, vmin, vmax, 0, 100, None, None, ops)
    return _render(d, m, vmm, cmap, invalid_val, background_color, gamma_corrected, value_transform, "rgba", ops)


def depth_to_uint16(depth, ops=None):
    """tester.py:75: (depth * 256).astype('uint16') -> torch.uint16 [H,W] on the device."""
    ops = ops or _ops()
    d = _plane(depth)
    return ops.depth_to_u16(d, torch.empty(d.shape, dtype=torch.uint16, device=d.device))


def _png_chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(data, zlib.crc32(kind)))


PNG_STRATEGIES = ("huffman", "rle", "auto")


def png_cost_bits(counts, table, nsym, header_bits, nbands, extra_bits=0):
    """Exact size in bits of the deflate blocks a table gives: sum of count * code length, the matches' extra bits and one distance
    bit each (symbols from 257 up), and per band the header, the end-of-block (in counts) and the empty stored block of the flush."""
    bits = sum(int(c) * (int(t) >> 16) for c, t in zip(counts[:nsym], table[:nsym]))
    return bits + int(extra_bits) + sum(int(c) for c in counts[257:nsym]) + nbands * (int(header_bits) + 3 + 32)


def encode_png(image, bgr=False, strategy="huffman", ops=None):
    """A device image -> the bytes of a PNG file.  image: uint8 [H,W], [H,W,3], [H,W,4] (grey, RGB, RGBA) or torch.uint16 [H,W];
    bgr=True reads channels 0 and 2 swapped, so `colorize(..., layout='bgr')` (the array cv2.imwrite takes, tester.py:69-72) gives the
    file cv2 writes.  Row filters, histogram, Huffman coding and compaction run on the device (csrc/png.hip); the host builds the code
    table from 257 counts (1 KB down, 1.3 KB up), reads the band sizes and Adler-32 partial sums (12 bytes per band of 8 rows) and the
    compressed bytes, combines the Adler-32 and computes the chunk CRC-32s over the compressed bytes: container checksums, not compute.
    strategy: 'huffman' codes every filtered byte as a literal; 'rle' adds matches at distance 1 for runs of equal bytes inside a row
    (csrc/png_rle.hip: smaller colour files, larger 16-bit ones); 'auto' builds both tables from one histogram download and encodes
    with the one whose exact bit cost is smaller (a tie goes to 'huffman')."""
    if strategy not in PNG_STRATEGIES:
        raise ValueError(f"png: strategy must be one of {PNG_STRATEGIES}, got {strategy!r}")
    ops = ops or _ops()
    img = image.detach().contiguous()
    H, W, ch, bits, _ = ops.png_format(img, bgr)
    dev = img.device
    if strategy == "huffman":
        ws_bytes, out_bytes, nbands = ops.png_workspace(img, bgr)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        hist = torch.empty(257, dtype=torch.int32, device=dev)
        ops.png_filter_histogram(img, ws, hist, bgr)
        table = ops.png_build_table(hist.cpu().numpy().view(np.uint32))
        encode = ops.png_encode
    else:
        ws_bytes, out_bytes, nbands = ops.png_rle_workspace(img, bgr)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        hist = torch.empty(ops.PNG_RLE_HIST_WORDS, dtype=torch.int32, device=dev)
        ops.png_rle_filter_histogram(img, ws, hist, bgr)
        h = hist.cpu().numpy().view(np.uint32)
        tokens = h[257:257 + 286]
        table = ops.png_rle_build_table(tokens)
        encode = ops.png_rle_encode
        if strategy == "auto":
            literal_table = ops.png_build_table(h[:257])
            rle_bits = png_cost_bits(tokens, table, 286, table[286], nbands, int(h[544]) | (int(h[545]) << 32))
            if png_cost_bits(h[:257], literal_table, 257, literal_table[257], nbands) <= rle_bits:
                table, encode = literal_table, ops.png_encode
    out = torch.empty(out_bytes, dtype=torch.uint8, device=dev)
    meta = torch.empty(2 + 3 * nbands, dtype=torch.int32, device=dev)
    encode(img, torch.from_numpy(table.view(np.int32)).to(dev), ws, out, meta, bgr)
    m = meta.cpu().numpy().view(np.uint32).tolist()
    total = m[0] | (m[1] << 32)
    assert total == sum(m[2::3]) and total <= out_bytes, (total, out_bytes)
    body = out[:total].cpu().numpy().tobytes()
    a, b, stride = 1, 0, W * ch * bits // 8 + 1
    for k in range(nbands):                                                 # Adler-32 of the whole stream from the band partials
        n = min(ops.PNG_BAND_ROWS, H - k * ops.PNG_BAND_ROWS) * stride
        b += n * a + m[2 + 3 * k + 2]
        a += m[2 + 3 * k + 1]
    adler = ((b % 65521) << 16) | (a % 65521)
    idat = b"\x78\x01" + body + b"\x01\x00\x00\xff\xff" + struct.pack(">I", adler)     # zlib header, bands, final empty stored block
    ihdr = struct.pack(">IIBBBBB", W, H, bits, {1: 0, 3: 2, 4: 6}[ch], 0, 0, 0)
    return b"\x89PNG\r\n\x1a\n" + _png_chunk(b"IHDR", ihdr) + _png_chunk(b"IDAT", idat) + _png_chunk(b"IEND", b"")


def save_prediction(result, work_dir, basename, gray_scale=False, ops=None, png_strategy="huffman"):
    """tester.py:66-76 with both encodes on the device: `{basename}.png` decodes to colorize(result, cmap='magma_r' | 'gray_r')[..., :3]
    (what cv2.imwrite makes of the BGR array) and `{basename}_uint16.png` to (depth * 256).astype('uint16').  png_strategy is
    encode_png's `strategy` for both files ('auto' picks per file).  -> the two paths."""
    ops = ops or _ops()
    colour = colorize(result, cmap="gray_r" if gray_scale else "magma_r", ops=ops, layout="bgr")
    colour_path = os.path.join(work_dir, f"{basename}.png")
    uint16_path = os.path.join(work_dir, f"{basename}_uint16.png")
    with open(colour_path, "wb") as f:
        f.write(encode_png(colour, bgr=True, strategy=png_strategy, ops=ops))
    with open(uint16_path, "wb") as f:
        f.write(encode_png(depth_to_uint16(result, ops=ops), strategy=png_strategy, ops=ops))
    return colour_path, uint16_path


def crop_rectangle(gh, gw, garg_crop, eigen_crop, dataset):
    """estimator/utils/metric.py:113-126 -> rows [y0,y1), cols [x0,x1) of the evaluation mask."""
    if garg_crop:
        return int(0.40810811 * gh), int(0.99189189 * gh), int(0.03594771 * gw), int(0.96405229 * gw)
    if eigen_crop:
        if dataset == "kitti":
            return int(0.3324324 * gh), int(0.91351351 * gh), int(0.0359477 * gw), int(0.96405229 * gw)
        return 45, 471, 41, 601
    return 0, gh, 0, gw


def metrics_from_sums(s):
    """13 accumulated sums (include/pf_hip.h: pf_depth_metrics) -> the reference's metric dict (metric.py:30-52,136-146)."""
    n = s[0]
    if n <= 0:
        nan = float("nan")
        r = dict(a1=nan, a2=nan, a3=nan, abs_rel=nan, rmse=nan, log_10=nan, rmse_log=nan, silog=nan, sq_rel=nan)
    else:
        var = s[9] / n - (s[8] / n) ** 2
        r = dict(a1=s[1] / n, a2=s[2] / n, a3=s[3] / n, abs_rel=s[4] / n, rmse=math.sqrt(s[6] / n), log_10=s[10] / n,
                 rmse_log=math.sqrt(s[7] / n), silog=(math.sqrt(var) if var >= 0 else float("nan")) * 100, sq_rel=s[5] / n)
    return r


def compute_metrics(gt, pred, interpolate=True, garg_crop=False, eigen_crop=True, dataset="nyu", min_depth_eval=0.1, max_depth_eval=10,
                    disp_gt_edges=None, additional_mask=None, ops=None):
    """estimator/utils/metric.py:87-148 on the device (signature and defaults of the reference).  pred is resized to
    the ground-truth grid inside the kernel when `interpolate` and the grids differ."""
    ops = ops or _ops()
    g, p = _plane(gt), _plane(pred)
    if g.shape != p.shape and not interpolate:
        raise ValueError("gt and pred grids differ and interpolate=False")
    e = None
    if disp_gt_edges is not None:
        e = _plane(disp_gt_edges.to(g.device))
    am = None
    if additional_mask is not None:                                           # metric.py:128-130 (prompt-depth evaluation)
        am = (_plane_any(additional_mask.to(g.device)) != 0).to(torch.uint8).contiguous()
    out = torch.empty(13, dtype=torch.float64, device=g.device)
    ops.depth_metrics(g, p, e, min_depth_eval, max_depth_eval, crop_rectangle(g.shape[0], g.shape[1], garg_crop, eigen_crop, dataset), out,
                      additional_mask=am)
    s = out.cpu().tolist()
    r = metrics_from_sums(s)
    if disp_gt_edges is not None:
        r["see"] = s[11] / s[12] if s[12] > 0 else 0.0
    return r


def get_boundaries(disp, th=1., dilation=10, ops=None):
    """estimator/utils/image_ops.py:25-36 (= utils/metric.py:74-85) on the device: -> float32 tensor [H,W] of 0 / 1, the `disp_gt_edges`
    of compute_metrics.  1 where the disparity differs from an up / down / left / right neighbour by more than th; dilation k > 0
    then dilates by a k x k box like cv2.dilate (anchor (k//2, k//2); 0 <= k <= 32, ValueError beyond)."""
    ops = ops or _ops()
    d = _plane(disp)
    return ops.depth_boundaries(d, th, dilation, torch.empty_like(d))


METRIC_KEYS = ("a1", "a2", "a3", "abs_rel", "rmse", "log_10", "rmse_log", "silog", "sq_rel", "see")


class DepthEvaluator:
    """The per-dataset evaluation loop (Tester.run -> dataset.get_metrics per image, dataset.evaluate -> pre_eval_to_metrics at the end,
    u4k_dataset.py:185-213) without a host synchronisation per image: add() only queues kernels on the current stream, the 13 sums of
    every image stay in one device buffer and results() / summary() fetch all of them with a single copy."""

    def __init__(self, min_depth_eval, max_depth_eval, garg_crop=False, eigen_crop=False, dataset="", capacity=64, ops=None):
        self.min_depth_eval, self.max_depth_eval = float(min_depth_eval), float(max_depth_eval)
        self.garg_crop, self.eigen_crop, self.dataset = garg_crop, eigen_crop, dataset
        self.capacity = max(1, int(capacity))
        self._ops = ops
        self._buf = None                       # [capacity, 13] float64 on the device of the first image
        self._has_edges = []                   # per image, host side

    def __len__(self):
        return len(self._has_edges)

    def add(self, depth_gt, pred, disp_gt=None, disp_gt_edges=None, additional_mask=None, th=1., dilation=0):
        """Queue the metrics of one image (compute_metrics' arithmetic, pred resized to the ground-truth grid inside the kernel) into the
        next row of the device buffer; with disp_gt instead of ready-made disp_gt_edges the boundary plane is made by get_boundaries
        (th, dilation) first.  Performs NO host synchronisation and NO device-to-host copy as long as every tensor passed in already
        lives on the device (a host tensor would have to be uploaded, which blocks); returns the index of the image."""
        ops = self._ops or _ops()
        g, p = _plane(depth_gt), _plane(pred)
        e = None
        if disp_gt_edges is not None:
            e = _plane(disp_gt_edges.to(g.device))
        elif disp_gt is not None:
            e = get_boundaries(disp_gt.to(g.device), th, dilation, ops=ops)
        if e is not None and e.shape != g.shape:
            raise ValueError(f"edge plane {tuple(e.shape)} and ground truth {tuple(g.shape)} differ")
        am = None
        if additional_mask is not None:
            am = (_plane_any(additional_mask.to(g.device)) != 0).to(torch.uint8).contiguous()
        i = len(self._has_edges)
        if self._buf is None:
            self._buf = torch.zeros(self.capacity, 13, dtype=torch.float64, device=g.device)
        elif i == self._buf.shape[0]:                                          # full: reallocate and copy on the device
            self.capacity *= 2
            buf = torch.zeros(self.capacity, 13, dtype=torch.float64, device=self._buf.device)
            buf[:i].copy_(self._buf)
            self._buf = buf
        ops.depth_metrics(g, p, e, self.min_depth_eval, self.max_depth_eval,
                          crop_rectangle(g.shape[0], g.shape[1], self.garg_crop, self.eigen_crop, self.dataset), self._buf[i], additional_mask=am)
        self._has_edges.append(e is not None)
        return i

    def results(self):
        """one device-to-host copy -> the list of dicts compute_metrics would have returned, image by image"""
        n = len(self._has_edges)
        if n == 0:
            return []
        out = []
        for s, has_edges in zip(self._buf[:n].cpu().tolist(), self._has_edges):
            r = metrics_from_sums(s)
            if has_edges:
                r["see"] = s[11] / s[12] if s[12] > 0 else 0.0
            out.append(r)
        return out

    def summary(self):
        """pre_eval_to_metrics (u4k_dataset.py:188-213): np.nanmean of every metric over the images, in the reference's key order.
        `see` is averaged over the images that were given edges and left out when none was (the reference requires edges everywhere)."""
        import warnings
        res = self.results()
        ret = {}
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)                    # "Mean of empty slice": nan, as in the reference
            for k in METRIC_KEYS:
                v = [r[k] for r in res if k in r]
                if v or k != "see":
                    ret[k] = float(np.nanmean(v)) if v else float("nan")
        return ret
