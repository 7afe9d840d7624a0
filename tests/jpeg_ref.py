"""NumPy restatement of the baseline JPEG decoder (csrc/jpeg_host.h, csrc/jpeg.hip): a marker parser, a sequential entropy decoder, a
model of the subsequence rounds of the device entropy decoder, and libjpeg's integer reconstruction (jidctint.c islow, jdsample.c fancy
upsampling, jdcolor.c).  tests/test_jpeg_ref_cpu.py pins it against PIL (libjpeg-turbo); the C and HIP code is then pinned against it.
Slow: small images only."""
import io
import os

import numpy as np

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg_cases.npz")


def load_cases():
    """-> dict name -> (jpeg bytes, expected uint8 [H,W,3] or None for the files that must be refused)"""
    z = np.load(GOLDEN)
    names = sorted(k[5:] for k in z.files if k.startswith("jpeg_"))
    return {n: (z["jpeg_" + n].tobytes(), z["rgb_" + n] if "rgb_" + n in z.files else None) for n in names}


class Header:
    pass


def parse(data):
    """markers up to the scan (supported files only) -> Header"""
    h = Header()
    h.qt, h.huff, h.dri, h.orientation = {}, {}, 0, 1
    assert data[:2] == b"\xff\xd8"
    p = 2
    while True:
        assert data[p] == 0xff
        m = data[p + 1]
        n = (data[p + 2] << 8) | data[p + 3]
        q = data[p + 4:p + 2 + n]
        p += 2 + n
        if m == 0xdb:
            o = 0
            while o < len(q):
                assert q[o] >> 4 == 0
                t = np.zeros(64, dtype=np.int64)
                t[ZIGZAG] = np.frombuffer(q[o + 1:o + 65], dtype=np.uint8)
                h.qt[q[o] & 15] = t
                o += 65
        elif m == 0xc4:
            o = 0
            while o < len(q):
                bits = list(q[o + 1:o + 17])
                tot = sum(bits)
                h.huff[(q[o] >> 4, q[o] & 15)] = (bits, list(q[o + 17:o + 17 + tot]))
                o += 17 + tot
        elif m in (0xc0, 0xc1):
            assert q[0] == 8
            h.height, h.width, h.ncomp = (q[1] << 8) | q[2], (q[3] << 8) | q[4], q[5]
            h.comps = [(q[6 + 3 * c], q[7 + 3 * c] >> 4, q[7 + 3 * c] & 15, q[8 + 3 * c]) for c in range(h.ncomp)]
        elif m == 0xdd:
            h.dri = (q[0] << 8) | q[1]
        elif m == 0xe1 and q[:6] == b"Exif\0\0":
            t = q[6:]
            bo = "<" if t[:2] == b"II" else ">"
            ifd = int(np.frombuffer(t[4:8], dtype=bo + "u4")[0])
            for i in range(int(np.frombuffer(t[ifd:ifd + 2], dtype=bo + "u2")[0])):
                e = t[ifd + 2 + 12 * i:ifd + 14 + 12 * i]
                if int(np.frombuffer(e[:2], dtype=bo + "u2")[0]) == 0x0112:
                    v = int(np.frombuffer(e[8:10], dtype=bo + "u2")[0])
                    h.orientation = v if 1 <= v <= 8 else 1
        elif m == 0xda:
            assert q[0] == h.ncomp
            h.tabs = [(q[2 + 2 * c] >> 4, q[2 + 2 * c] & 15) for c in range(h.ncomp)]
            h.scan_begin = p
            break
    if h.ncomp == 1:
        h.samp = [(1, 1)]
    else:
        h.samp = [(c[1], c[2]) for c in h.comps]
    h.hmax, h.vmax = h.samp[0]
    h.mcus_x = -(-h.width // (8 * h.hmax))
    h.mcus_y = -(-h.height // (8 * h.vmax))
    h.comp_of = [c for c in range(h.ncomp) for _ in range(h.samp[c][0] * h.samp[c][1])]
    h.bpm = len(h.comp_of)
    h.nblocks = h.mcus_x * h.mcus_y * h.bpm
    return h


def prepare_scan(data, h):
    """-> (unstuffed scan bytes, [(first bit, end bit) per restart interval])"""
    out, segs, start, p = bytearray(), [], 0, h.scan_begin
    while True:
        b = data[p]
        p += 1
        if b != 0xff:
            out.append(b)
            continue
        m = data[p]
        p += 1
        if m == 0:
            out.append(0xff)
        elif 0xd0 <= m <= 0xd7:
            segs.append((start, 8 * len(out)))
            start = 8 * len(out)
        elif m == 0xd9:
            segs.append((start, 8 * len(out)))
            return bytes(out), segs
        else:
            raise ValueError("marker in scan")


class Huff:
    def __init__(self, bits, vals):
        """look[16-bit window] = code length << 8 | symbol, 0 = no code"""
        self.look = np.zeros(1 << 16, dtype=np.int64)
        code, k = 0, 0
        for l in range(1, 17):
            for _ in range(bits[l - 1]):
                self.look[code << (16 - l):(code + 1) << (16 - l)] = (l << 8) | vals[k]
                code += 1
                k += 1
            code <<= 1
        self.look = self.look.tolist()


class Decoder:
    """one decoder step on the state (p, b, k) exactly as the device kernels take it"""

    def __init__(self, h, scan):
        self.h = h
        bits = np.unpackbits(np.frombuffer(scan + b"\0" * 8, dtype=np.uint8)).astype(np.int64)
        n = len(bits) - 16
        self.w16 = sum(bits[i:i + n] << (15 - i) for i in range(16)).tolist()          # the 16 bits from every bit position on
        self.dc = [Huff(*h.huff[(0, h.tabs[c][0])]) for c in range(h.ncomp)]
        self.ac = [Huff(*h.huff[(1, h.tabs[c][1])]) for c in range(h.ncomp)]

    def run(self, p, b, k, end, seg_end, sink=None, blk=0):
        """decode while p < end -> (p, b, k, blocks completed); sink(blk, index, value) receives the coefficients"""
        n = 0
        w16, comp_of, bpm = self.w16, self.h.comp_of, self.h.bpm
        while p < end:
            e = (self.ac if k else self.dc)[comp_of[b]].look[w16[p]]
            if not e:                      # no such code: one bit consumed, nothing set
                p += 1
                continue
            ln, sym = e >> 8, e & 255
            s, r = sym & 15, (sym >> 4) if k else 0
            if p + ln + s > seg_end:
                break
            v = w16[p + ln] >> (16 - s) if s else 0
            if s and v < (1 << (s - 1)):
                v -= (1 << s) - 1
            p += ln + s
            if k == 0:
                if sink:
                    sink(blk, 0, v)
                k = 1
            elif s == 0:
                k = k + 16 if r == 15 else 64
            else:
                k += r
                if sink:
                    sink(blk, int(ZIGZAG[min(k, 63)]), v)
                k += 1
            if k >= 64:
                k, b, n, blk = 0, (b + 1) % bpm, n + 1, blk + 1
        return p, b, k, n


def seg_blocks(h, nseg, s):
    per = h.dri * h.bpm if h.dri else h.nblocks
    return min(per, h.nblocks - per * s)


def decode_entropy(data, h=None):
    """sequential decoder -> int16 [nblocks, 64] in the coefficient layout (natural order, not dequantised, DC absolute)"""
    h = h or parse(data)
    scan, segs = prepare_scan(data, h)
    d = Decoder(h, scan)
    coef = np.zeros((h.nblocks, 64), dtype=np.int64)

    def sink(blk, i, v):
        coef[blk, i] = v

    per = h.dri * h.bpm if h.dri else h.nblocks
    for s, (a, e) in enumerate(segs):
        p, b, k, blk = a, 0, 0, per * s
        for _ in range(seg_blocks(h, len(segs), s)):
            p, b, k, n = d.run(p, b, k, p + 1, e, sink, blk)       # one symbol at a time up to the block's end
            while k:
                p0 = p
                p, b, k, n = d.run(p, b, k, p + 1, e, sink, blk)
                assert p > p0, "stream error"
            blk += 1
        assert b == 0 and 0 <= e - p <= 7
        pred = [0] * h.ncomp
        for j in range(per * s, per * s + seg_blocks(h, len(segs), s)):
            c = h.comp_of[j % h.bpm]
            pred[c] += coef[j, 0]
            coef[j, 0] = pred[c]
    return coef.astype(np.int16)


def sync_model(data, S, h=None, max_rounds=None):
    """the subsequence rounds of the device decoder -> (exit states after convergence, rounds run, true exit states).  A round re-decodes
    every lane that is not the first of its segment from the exit state the lane before it had after the round before; the loop ends
    after a round that changes nothing, after (longest segment in lanes) - 1 rounds, or after max_rounds rounds (then the states
    returned are not converged; the true states are still computed)."""
    h = h or parse(data)
    scan, segs = prepare_scan(data, h)
    d = Decoder(h, scan)
    lanes = []
    for s, (a, e) in enumerate(segs):
        cnt = max(1, -(-(e - a) // S))
        lanes += [(a + i * S, min(a + i * S + S, e), e, i == 0) for i in range(cnt)]
    longest = max(max(1, -(-(e - a) // S)) for a, e in segs)
    cur = [d.run(st, 0, 0, en, se) for st, en, se, _ in lanes]
    entry = [(st, 0, 0) for st, en, se, _ in lanes]
    truth = []
    for i, (st, en, se, head) in enumerate(lanes):
        truth.append(d.run(st, 0, 0, en, se) if head else d.run(*truth[-1][:3], en, se))
    rounds = 0
    for r in range(1, longest):
        nxt = list(cur)
        for i in range(len(lanes)):
            if not lanes[i][3] and cur[i - 1][:3] != entry[i]:          # a lane whose entry state did not change keeps its exit state
                entry[i] = cur[i - 1][:3]
                nxt[i] = d.run(*entry[i], lanes[i][1], lanes[i][2])
        rounds = r
        changed = nxt != cur
        cur = nxt
        if not changed or r == max_rounds:
            break
    return cur, rounds, truth


# ------------------------------------------------------------------------------------------------ reconstruction
F = dict(f0_298=2446, f0_390=3196, f0_541=4433, f0_765=6270, f0_899=7373, f1_175=9633, f1_501=12299, f1_847=15137, f1_961=16069,
         f2_053=16819, f2_562=20995, f3_072=25172)


def _idct_pass(x):
    """jpeg_idct_islow's one-dimensional pass along axis 1 of [n, 8] -> [n, 8], not descaled"""
    i = [x[:, j] for j in range(8)]
    z1 = (i[2] + i[6]) * F["f0_541"]
    t2 = z1 - i[6] * F["f1_847"]
    t3 = z1 + i[2] * F["f0_765"]
    t0 = (i[0] + i[4]) * 8192
    t1 = (i[0] - i[4]) * 8192
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    a0, a1, a2, a3 = i[7], i[5], i[3], i[1]
    z1, z2, z3, z4 = a0 + a3, a1 + a2, a0 + a2, a1 + a3
    z5 = (z3 + z4) * F["f1_175"]
    a0, a1, a2, a3 = a0 * F["f0_298"], a1 * F["f2_053"], a2 * F["f3_072"], a3 * F["f1_501"]
    z1, z2, z3, z4 = -z1 * F["f0_899"], -z2 * F["f2_562"], -z3 * F["f1_961"] + z5, -z4 * F["f0_390"] + z5
    a0, a1, a2, a3 = a0 + z1 + z3, a1 + z2 + z4, a2 + z2 + z3, a3 + z1 + z4
    return np.stack([t10 + a3, t11 + a2, t12 + a1, t13 + a0, t13 - a0, t12 - a1, t11 - a2, t10 - a3], axis=1)


def idct_blocks(coef, qt):
    """int16 [n, 64] x quantisation table [64] -> uint8 [n, 8, 8]"""
    x = (coef.astype(np.int64) * qt[None, :]).reshape(-1, 8, 8)
    n = x.shape[0]
    cols = x.transpose(0, 2, 1).reshape(-1, 8)                                  # column pass, descale 11
    w = ((_idct_pass(cols) + (1 << 10)) >> 11).reshape(n, 8, 8).transpose(0, 2, 1)
    rows = ((_idct_pass(w.reshape(-1, 8)) + (1 << 17)) >> 18).reshape(n, 8, 8)  # row pass, descale 18
    return np.clip(rows + 128, 0, 255).astype(np.uint8)


def planes_from_coef(h, coef):
    """-> one uint8 plane per component, padded to whole MCUs"""
    planes = []
    blocks = coef.reshape(h.mcus_y, h.mcus_x, h.bpm, 64)
    b0 = 0
    for c in range(h.ncomp):
        ch, cv = h.samp[c]
        px = idct_blocks(blocks[:, :, b0:b0 + ch * cv].reshape(-1, 64), h.qt[h.comps[c][3]])
        px = px.reshape(h.mcus_y, h.mcus_x, cv, ch, 8, 8).transpose(0, 2, 4, 1, 3, 5).reshape(h.mcus_y * cv * 8, h.mcus_x * ch * 8)
        planes.append(px)
        b0 += ch * cv
    return planes


def upsample(pl, h, c):
    """fancy upsampling of component c to [H, W] int"""
    H, W = h.height, h.width
    ch, cv = h.samp[c]
    if ch == h.hmax and cv == h.vmax:
        return pl[:H, :W].astype(np.int64)
    sw, sh = -(-W * ch // h.hmax), -(-H * cv // h.vmax)
    s = pl[:sh, :sw].astype(np.int64)
    x = np.arange(W)
    col = x >> 1
    left, right = np.maximum(col - 1, 0), np.minimum(col + 1, sw - 1)
    if h.vmax == 1:                                                           # h2v1
        t = s[:, col]
        even = np.where(col == 0, t, (3 * t + s[:, left] + 1) >> 2)
        odd = np.where(col == sw - 1, t, (3 * t + s[:, right] + 2) >> 2)
        return np.where((x & 1) == 1, odd, even)
    y = np.arange(H)
    r = y >> 1
    near = np.where((y & 1) == 1, np.minimum(r + 1, sh - 1), np.maximum(r - 1, 0))
    cs = 3 * s[r] + s[near]                                                   # [H, sw] column sums
    t = cs[:, col]
    even = np.where(col == 0, (4 * t + 8) >> 4, (3 * t + cs[:, left] + 8) >> 4)
    odd = np.where(col == sw - 1, (4 * t + 7) >> 4, (3 * t + cs[:, right] + 7) >> 4)
    return np.where((x & 1) == 1, odd, even)


def orient(a, o):
    """EXIF orientation o applied to [H, W, 3] (what ImageOps.exif_transpose and cv2.imread do)"""
    if o == 2:
        return a[:, ::-1]
    if o == 3:
        return a[::-1, ::-1]
    if o == 4:
        return a[::-1]
    if o == 5:
        return a.transpose(1, 0, 2)
    if o == 6:
        return a.transpose(1, 0, 2)[:, ::-1]
    if o == 7:
        return a[::-1, ::-1].transpose(1, 0, 2)
    if o == 8:
        return a.transpose(1, 0, 2)[::-1]
    return a


def reconstruct(h, coef, orientation=1):
    """coefficient array -> uint8 [H', W', 3] RGB"""
    planes = planes_from_coef(h, coef)
    y = upsample(planes[0], h, 0)
    if h.ncomp == 1:
        rgb = np.stack([y, y, y], axis=-1)
    else:
        cb, cr = upsample(planes[1], h, 1) - 128, upsample(planes[2], h, 2) - 128
        rgb = np.stack([y + ((91881 * cr + 32768) >> 16), y + ((-22554 * cb - 46802 * cr + 32768) >> 16), y + ((116130 * cb + 32768) >> 16)], axis=-1)
    return np.ascontiguousarray(orient(np.clip(rgb, 0, 255).astype(np.uint8), orientation))


def decode(data, apply_orientation=True):
    h = parse(data)
    return reconstruct(h, decode_entropy(data, h), h.orientation if apply_orientation else 1)


# ------------------------------------------------------------------------------------------------ inputs
def image(kind, H, W, seed, grey=False):
    """seeded test content: 'noise' (uniform bytes) or 'smooth' (low-frequency waves + a hard edge)"""
    rng = np.random.default_rng(seed)
    if kind == "noise":
        a = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    else:
        yy, xx = np.mgrid[0:H, 0:W]
        ph = rng.uniform(0, 6.28, (3, 2))
        a = np.stack([127 + 90 * np.sin(xx / (7.0 + 3 * c) + ph[c, 0]) * np.cos(yy / (9.0 + 2 * c) + ph[c, 1]) for c in range(3)], axis=-1)
        a[H // 3:, W // 2:] = 255 - a[H // 3:, W // 2:]
        a = np.clip(a, 0, 255).astype(np.uint8)
    return a[..., 0] if grey else a


def pil_encode(a, quality=90, subsampling="4:2:0", optimize=False, restart_blocks=0, restart_rows=0, progressive=False, exif=None):
    from PIL import Image
    buf = io.BytesIO()
    kw = dict(quality=quality, optimize=optimize, progressive=progressive)
    if a.ndim == 3:
        kw["subsampling"] = subsampling
    if restart_blocks:
        kw["restart_marker_blocks"] = restart_blocks
    if restart_rows:
        kw["restart_marker_rows"] = restart_rows
    if exif is not None:
        kw["exif"] = exif
    Image.fromarray(a).save(buf, "JPEG", **kw)
    return buf.getvalue()


def pil_decode(data, transpose=False):
    from PIL import Image, ImageOps
    im = Image.open(io.BytesIO(data))
    if transpose:
        im = ImageOps.exif_transpose(im)
    return np.asarray(im.convert("RGB"))
