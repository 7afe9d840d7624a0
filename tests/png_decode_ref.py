"""Slow, plain side of the PNG decoder tests, on NumPy and the standard library's zlib: a decoder (chunk parse, zlib, unfilter, expand), a
writer (any colour type and depth, filter types given per row, zlib's level / memLevel / strategy, composite streams made of sync-flushed
pieces, hand-assembled fixed-Huffman blocks) and a model of the device algorithm of csrc/png_decode.hip (finder, scan records, chain walk
with its rounds, references with in-block following, pointer jumping).  Nothing here is fast or clever on purpose: it is the reference."""
import os
import struct
import zlib

import numpy as np

SIGNATURE = b"\x89PNG\r\n\x1a\n"
CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}
PAIRS = [(0, 1), (0, 2), (0, 4), (0, 8), (0, 16), (2, 8), (2, 16), (3, 1), (3, 2), (3, 4), (3, 8), (4, 8), (4, 16), (6, 8), (6, 16)]
S_OK, S_INVALID, S_LIMIT, S_EOS, S_SIZE, S_DIST = range(6)
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LEN_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289,
             16385, 24577)
DIST_EXTRA = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "png_decode_cases.npz")


# ---------------------------------------------------------------- decoder
def chunks(png):
    """[(type, data)] of a PNG file; CRCs are not looked at"""
    assert png[:8] == SIGNATURE
    pos, out = 8, []
    while pos + 12 <= len(png):
        n, kind = struct.unpack(">I4s", png[pos:pos + 8])
        out.append((kind, png[pos + 8:pos + 8 + n]))
        pos += 12 + n
    return out


def parse(png):
    h = dict(palette=None, has_trns=False)
    idat = []
    for kind, data in chunks(png):
        if kind == b"IHDR":
            h["width"], h["height"], h["depth"], h["color_type"], _, _, h["interlace"] = struct.unpack(">IIBBBBB", data)
        elif kind == b"PLTE":
            h["palette"] = np.frombuffer(data, dtype=np.uint8).reshape(-1, 3)
        elif kind == b"tRNS":
            h["has_trns"] = True
        elif kind == b"IDAT":
            idat.append(data)
    h["channels"] = CHANNELS[h["color_type"]]
    bits = h["channels"] * h["depth"]
    h["bpp"] = max(1, bits // 8)
    h["rowbytes"] = (h["width"] * bits + 7) // 8
    h["idat"] = b"".join(idat)
    return h


def _paeth(a, b, c):
    pa, pb, pc = abs(b - c), abs(a - c), abs(a + b - 2 * c)
    return a if (pa <= pb and pa <= pc) else (b if pb <= pc else c)


def unfilter(raw, height, rowbytes, bpp):
    """the filtered bytes [height * (1 + rowbytes)] -> uint8 [height, rowbytes], exact per the specification"""
    raw = np.frombuffer(bytes(raw), dtype=np.uint8).reshape(height, 1 + rowbytes)
    out = np.zeros((height, rowbytes), dtype=np.uint8)
    prev = [0] * rowbytes
    for y in range(height):
        f, line = int(raw[y, 0]), raw[y, 1:].tolist()
        assert f <= 4, f
        cur = [0] * rowbytes
        for i, v in enumerate(line):
            a = cur[i - bpp] if i >= bpp else 0
            b = prev[i]
            c = prev[i - bpp] if i >= bpp else 0
            pred = (0, a, b, (a + b) >> 1, _paeth(a, b, c))[f]
            cur[i] = (v + pred) & 255
        out[y] = cur
        prev = cur
    return out


def expand(rows, h):
    """the unfiltered rows -> the array decode_png returns"""
    H, W, depth, ct, ch = h["height"], h["width"], h["depth"], h["color_type"], h["channels"]
    if depth == 16:
        a = rows.reshape(H, W * ch, 2).astype(np.uint16)
        a = (a[..., 0] << 8) | a[..., 1]
    elif depth == 8:
        a = rows
    else:
        bits = np.unpackbits(rows, axis=1)[:, :W * depth].reshape(H, W, depth)
        a = np.zeros((H, W), dtype=np.uint8)
        for k in range(depth):
            a = (a << 1) | bits[..., k]
        if ct == 0:
            a = a * (255 // ((1 << depth) - 1))
    if ct == 3:
        return h["palette"][a.reshape(H, W)]
    a = a.astype(np.uint16 if depth == 16 else np.uint8)
    return a.reshape(H, W) if ch == 1 else a.reshape(H, W, ch)


def decode(png):
    h = parse(png)
    assert not h["interlace"]
    raw = zlib.decompress(h["idat"])
    assert len(raw) == h["height"] * (1 + h["rowbytes"])
    return expand(unfilter(raw, h["height"], h["rowbytes"], h["bpp"]), h)


def to_rgb8(a):
    """what ImagePreprocessor.read makes of a decoded PNG: grey replicated, alpha dropped, the high byte of 16-bit samples"""
    if a.dtype == np.uint16:
        a = (a >> 8).astype(np.uint8)
    if a.ndim == 2:
        a = a[..., None]
    return np.ascontiguousarray(a[..., [0, 0, 0]] if a.shape[2] < 3 else a[..., :3])


# ---------------------------------------------------------------- writer
def chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data))


def pack_rows(samples, depth):
    """integer samples [H, W, C] -> uint8 [H, rowbytes]: 16-bit big-endian, sub-byte samples from the high bits down"""
    s = np.asarray(samples)
    H = s.shape[0]
    s = s.reshape(H, -1)
    if depth == 16:
        return s.astype(">u2").view(np.uint8).reshape(H, -1)
    if depth == 8:
        return s.astype(np.uint8)
    bits = ((s[..., None].astype(np.uint8) >> np.arange(depth - 1, -1, -1)) & 1).reshape(H, -1)
    return np.packbits(bits.astype(np.uint8), axis=1)


def filter_rows(rows, bpp, filters):
    """uint8 [H, rowbytes] -> the filtered bytes, row y with type filters[y % len(filters)]"""
    H, n = rows.shape
    out = bytearray()
    prev = [0] * n
    for y in range(H):
        f, cur = filters[y % len(filters)], rows[y].tolist()
        out.append(f)
        for i, v in enumerate(cur):
            a = cur[i - bpp] if i >= bpp else 0
            b = prev[i]
            c = prev[i - bpp] if i >= bpp else 0
            out.append((v - (0, a, b, (a + b) >> 1, _paeth(a, b, c))[f]) & 255)
        prev = cur
    return bytes(out)


def write_png(samples, color_type, depth, filters=(0,), level=6, mem_level=8, strategy=0, palette=None, trns=None, raw_deflate=None,
              filtered=None, interlace=0, zlib_header=None, adler=None, idat_split=None, extra_chunks=()):
    """samples: integers [H, W, C] (C = the colour type's channels; palette indices for type 3).  raw_deflate replaces the compressor's
    output (the zlib header and the Adler-32 of the filtered bytes are put around it); filtered replaces the filtered bytes."""
    s = np.asarray(samples)
    if s.ndim == 2:
        s = s[..., None]
    H, W = s.shape[:2]
    assert s.shape[2] == CHANNELS[color_type]
    if filtered is None:
        filtered = filter_rows(pack_rows(s, depth), max(1, CHANNELS[color_type] * depth // 8), filters)
    if raw_deflate is None:
        c = zlib.compressobj(level, zlib.DEFLATED, -15, mem_level, strategy)
        raw_deflate = c.compress(filtered) + c.flush()
    head = b"\x78\x9c" if zlib_header is None else zlib_header
    z = head + raw_deflate + struct.pack(">I", zlib.adler32(filtered) if adler is None else adler)
    out = SIGNATURE + chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, depth, color_type, 0, 0, interlace))
    for kind, data in extra_chunks:
        out += chunk(kind, data)
    if palette is not None:
        out += chunk(b"PLTE", np.asarray(palette, dtype=np.uint8).tobytes())
    if trns is not None:
        out += chunk(b"tRNS", bytes(trns))
    cuts = [0] + list(idat_split or []) + [len(z)]
    for a, b in zip(cuts[:-1], cuts[1:]):
        out += chunk(b"IDAT", z[a:b])
    return out + chunk(b"IEND", b"")


def composite_deflate(pieces):
    """pieces: [(bytes, dict(level=, mem_level=, strategy=))] -> one raw deflate stream: every piece is compressed on its own with the
    bytes before it as the dictionary (so matches cross pieces) and sync-flushed (which appends an empty stored block), the last finished"""
    out, seen = b"", b""
    for i, (data, kw) in enumerate(pieces):
        args = dict(level=kw.get("level", 6), method=zlib.DEFLATED, wbits=-15, memLevel=kw.get("mem_level", 8), strategy=kw.get("strategy", 0))
        c = zlib.compressobj(zdict=seen[-32768:], **args) if seen else zlib.compressobj(**args)
        out += c.compress(data) + c.flush(zlib.Z_FINISH if i == len(pieces) - 1 else zlib.Z_SYNC_FLUSH)
        seen += data
    return out


class BitWriter:
    """deflate bit order: the first bit written is bit 0 of byte 0"""

    def __init__(self):
        self.bits = []

    def put(self, value, n):                  # n bits, lowest first
        self.bits.extend((value >> b) & 1 for b in range(n))

    def code(self, value, n):                 # a Huffman code: highest bit first
        self.bits.extend((value >> b) & 1 for b in range(n - 1, -1, -1))

    def tobytes(self):
        bits = self.bits + [0] * (-len(self.bits) % 8)
        return np.packbits(np.array(bits, dtype=np.uint8), bitorder="little").tobytes()


def fixed_block(tokens, final=True, writer=None):
    """a fixed-Huffman block by hand: tokens are literals (int) or matches (length, distance)"""
    w = writer or BitWriter()
    w.put(1 if final else 0, 1)
    w.put(1, 2)

    def litlen(s):
        if s < 144:
            w.code(0x30 + s, 8)
        elif s < 256:
            w.code(0x190 + s - 144, 9)
        elif s < 280:
            w.code(s - 256, 7)
        else:
            w.code(0xc0 + s - 280, 8)

    for t in tokens:
        if isinstance(t, tuple):
            n, d = t
            k = max(i for i in range(29) if LEN_BASE[i] <= n and (i == 28 or n < 258))
            litlen(257 + k)
            w.put(n - LEN_BASE[k], LEN_EXTRA[k])
            k = max(i for i in range(30) if DIST_BASE[i] <= d)
            w.code(k, 5)
            w.put(d - DIST_BASE[k], DIST_EXTRA[k])
        else:
            litlen(int(t))
    litlen(256)
    return w


# ---------------------------------------------------------------- the device algorithm
class Bits:
    def __init__(self, data):
        self.data = bytes(data)
        self.nbits = 8 * len(self.data)
        padded = np.frombuffer(self.data + b"\0" * 8, dtype=np.uint8).astype(np.uint64)
        n = len(self.data) + 4
        self.w = (padded[0:n] | padded[1:n + 1] << 8 | padded[2:n + 2] << 16 | padded[3:n + 3] << 24).tolist()

    def peek(self, p, k):                     # k <= 25 bits at p, first bit lowest, zeros past the end
        if p >= self.nbits:
            return 0
        return (self.w[p >> 3] >> (p & 7)) & ((1 << k) - 1)


def _build(lens):
    """code lengths -> (15-bit lookup: symbol | length << 9, or -1; Kraft sum in units of 2^-15; symbols of non-zero length)"""
    lens = list(lens)
    count = [0] * 16
    for n in lens:
        count[n] += 1
    count[0] = 0
    kraft = sum(count[n] << (15 - n) for n in range(1, 16))
    table = np.full(1 << 15, -1, dtype=np.int32)
    if kraft > (1 << 15):
        return table, kraft, sum(count)
    code, nxt = 0, [0] * 16
    for n in range(1, 16):
        code = (code + count[n - 1]) << 1
        nxt[n] = code
    for s, n in enumerate(lens):
        if n:
            rev = int(format(nxt[n], f"0{n}b")[::-1], 2)
            nxt[n] += 1
            table[rev::1 << n] = s | (n << 9)
    return table, kraft, sum(count)


def _kraft_ok(kraft, nonzero, may_be_empty):
    return kraft == (1 << 15) or (nonzero == 1 and kraft == (1 << 14)) or (may_be_empty and nonzero == 0)


def read_codes(b, p):
    """the header of the fixed or dynamic block at p (its BFINAL bit) -> (lit table, dist table, first symbol bit) or None"""
    kind = b.peek(p, 3) >> 1
    p += 3
    if kind == 1:
        lens = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
        return _build(lens)[0].tolist(), _build([5] * 30)[0].tolist(), p
    if kind != 2:
        return None
    nlit, ndist, ncl = 257 + b.peek(p, 5), 1 + b.peek(p + 5, 5), 4 + b.peek(p + 10, 4)
    p += 14
    if nlit > 286 or ndist > 30:
        return None
    cl = [0] * 19
    for i in range(ncl):
        cl[CL_ORDER[i]] = b.peek(p, 3)
        p += 3
    table, kraft, _ = _build(cl)
    if kraft != (1 << 15):
        return None
    lens = []
    while len(lens) < nlit + ndist:
        e = int(table[b.peek(p, 15)])
        if e < 0:
            return None
        p += e >> 9
        s = e & 511
        if s < 16:
            lens.append(s)
        elif s == 16:
            if not lens:
                return None
            lens += [lens[-1]] * (3 + b.peek(p, 2))
            p += 2
        elif s == 17:
            lens += [0] * (3 + b.peek(p, 3))
            p += 3
        else:
            lens += [0] * (11 + b.peek(p, 7))
            p += 7
        if len(lens) > nlit + ndist or p > b.nbits:
            return None
    if not lens[256]:
        return None
    lit, kl, nl = _build(lens[:nlit])
    dist, kd, nd = _build(lens[nlit:])
    if not _kraft_ok(kl, nl, False) or not _kraft_ok(kd, nd, True):
        return None
    return lit.tolist(), dist.tolist(), p


def decode_block(b, p, stop, lit, dist, on_literal, on_match):
    """the symbol loop of png_inflate.h -> (status, bit behind the last symbol read)"""
    while p < stop:
        e = lit[b.peek(p, 15)]
        if e < 0:
            return S_INVALID, p
        p += e >> 9
        s = e & 511
        if s < 256:
            if not on_literal(s):
                return S_SIZE, p
            continue
        if s == 256:
            return (S_EOS if p > b.nbits else S_OK), p
        s -= 257
        if s > 28:
            return S_INVALID, p
        n = LEN_BASE[s] + b.peek(p, LEN_EXTRA[s])
        p += LEN_EXTRA[s]
        e = dist[b.peek(p, 15)]
        if e < 0 or (e & 511) > 29:
            return S_INVALID, p
        p += e >> 9
        d = DIST_BASE[e & 511] + b.peek(p, DIST_EXTRA[e & 511])
        p += DIST_EXTRA[e & 511]
        if p > b.nbits:
            return S_EOS, p
        st = on_match(n, d)
        if st != S_OK:
            return st, p
    return (S_EOS if stop >= b.nbits else S_LIMIT), p


def scan(b, start, max_bits, expected):
    """one candidate's record: (start, end bit, output bytes, status, BFINAL)"""
    codes = read_codes(b, start)
    if codes is None:
        return start, start, 0, S_INVALID, b.peek(start, 1)
    lit, dist, p = codes
    n = [0]

    def literal(_):
        n[0] += 1
        return n[0] <= expected

    def match(length, _):
        n[0] += length
        return S_OK if n[0] <= expected else S_SIZE

    st, end = decode_block(b, p, min(start + max_bits, b.nbits), lit, dist, literal, match)
    return start, end, n[0], st, b.peek(start, 1)


def find_candidates(deflate):
    """the finder: every bit offset at which a well-formed dynamic header starts (and offset 0 when a fixed block starts there).  The
    cheap parts of the test are vectorised; the survivors go through read_codes"""
    b = Bits(deflate)
    bits = np.unpackbits(np.frombuffer(bytes(deflate) + b"\0" * 16, dtype=np.uint8), bitorder="little").astype(np.int64)
    n = b.nbits

    def field(off, k):
        return sum(bits[off + j:off + j + n] << j for j in range(k))

    ok = (field(1, 2) == 2) & (field(3, 5) <= 29) & (field(8, 5) <= 29)
    ncl = 4 + field(13, 4)
    kraft = np.zeros(n, dtype=np.int64)
    for i in range(19):
        v = field(17 + 3 * i, 3) if 17 + 3 * i + 3 + n <= bits.size else np.zeros(n, dtype=np.int64)
        kraft += np.where((i < ncl) & (v > 0), 128 >> v, 0)
    out = [int(p) for p in np.nonzero(ok & (kraft == 128))[0] if read_codes(b, int(p)) is not None]
    if b.peek(0, 3) >> 1 == 1:
        out = [0] + out
    return out


def inflate_blocks(deflate, blocks, expected):
    """the inflate pass: blocks [(start, type, offset, bytes)] -> (lit uint8 [expected], ref int64 [expected], flags: 1 = a block did
    not decode to its size, 2 = a match reaches before the output).  A literal's reference is its own place; a matched byte gets the
    root of its source: ref[source] when the source lies in the same block, the source itself otherwise."""
    b = Bits(deflate)
    lit, ref, flags = np.zeros(expected, dtype=np.uint8), list(range(expected)), 0
    for start, kind, off, n in blocks:
        if off + n > expected:
            flags |= 1
            continue
        if kind == 0:
            if start + n > len(deflate):
                flags |= 1
                continue
            lit[off:off + n] = np.frombuffer(bytes(deflate[start:start + n]), dtype=np.uint8)
            continue
        o = [off]

        def literal(v):
            if o[0] >= off + n:
                return False
            lit[o[0]] = v
            o[0] += 1
            return True

        def match(length, d):
            if d > o[0]:
                return S_DIST
            if length > off + n - o[0]:
                return S_SIZE
            for _ in range(length):
                s = o[0] - d
                ref[o[0]] = ref[s] if s >= off else s            # in-block sources are followed at once
                o[0] += 1
            return S_OK

        codes = read_codes(b, start)
        st = S_INVALID if codes is None else decode_block(b, codes[2], b.nbits, codes[0], codes[1], literal, match)[0]
        if st == S_DIST:
            flags |= 2
        elif st != S_OK or o[0] != off + n:
            flags |= 1
    return lit, np.array(ref, dtype=np.int64), flags


def model(deflate, expected, max_block_bits=1 << 21, max_chain_rounds=8):
    """The device algorithm step by step -> dict(out=bytes or None, fallback=reason or None, candidates, blocks [(start, type, offset,
    bytes)], chain_rounds (scan passes), jump_rounds (the fixed count), jump_rounds_used (rounds that still changed a reference))"""
    b = Bits(deflate)
    cand = find_candidates(deflate)
    res = dict(out=None, fallback=None, candidates=cand, blocks=[], chain_rounds=0, jump_rounds=0, jump_rounds_used=0)
    if max_chain_rounds < 1:
        res["fallback"] = "rounds"
        return res
    table = {}
    queue, p, total = cand, 0, 0
    while True:
        res["chain_rounds"] += 1
        for c in queue:
            table[c] = scan(b, c, max_block_bits, expected)
        need = None
        while True:
            assert p + 3 <= b.nbits
            head = b.peek(p, 3)
            kind = head >> 1
            assert kind != 3
            if kind == 0:
                at = (p + 10) // 8
                n = deflate[at] | deflate[at + 1] << 8
                assert n ^ (deflate[at + 2] | deflate[at + 3] << 8) == 0xffff
                res["blocks"].append((at + 4, 0, total, n))
                p = 8 * (at + 4 + n)
            else:
                if p not in table:
                    assert kind == 1, "the finder missed a dynamic block"
                    need = p
                    break
                _, end, n, st, _ = table[p]
                if st == S_LIMIT:
                    res["fallback"] = "bits"
                    return res
                assert st == S_OK, st
                res["blocks"].append((p, kind, total, n))
                p = end
            total += n
            if head & 1:
                break
        if need is None:
            break
        if res["chain_rounds"] >= max_chain_rounds:
            res["fallback"] = "rounds"
            return res
        queue = [need]
    assert total == expected, (total, expected)
    lit, ref, flags = inflate_blocks(deflate, res["blocks"], expected)
    assert flags == 0, flags
    starts = np.array([k[2] for k in res["blocks"]] + [expected])
    block_of = np.searchsorted(starts, np.arange(expected), side="right") - 1
    assert np.all((ref == np.arange(expected)) | (block_of[ref] < block_of) | (ref[ref] == ref)), "a reference is neither a root nor earlier"
    res["jump_rounds"] = max(len(res["blocks"]) - 1, 0).bit_length() + 1
    for r in range(res["jump_rounds"]):
        nxt = ref[ref]
        if not np.array_equal(nxt, ref):
            res["jump_rounds_used"] = r + 1
        ref = nxt
    assert np.array_equal(ref[ref], ref)
    res["out"] = lit[ref].tobytes()
    return res


# ---------------------------------------------------------------- test images and cases
def photo(height, width, channels=3, seed=0, maximum=255, noise=4.0):
    """a seeded photo-like image: smooth gradients and waves with some noise"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:height, 0:width].astype(np.float64)
    planes = [0.5 + 0.25 * np.sin(x / (7.0 + 3 * c) + c) + 0.2 * np.cos(y / (5.0 + 2 * c)) + 0.1 * ((x + (c + 1) * y) % 37) / 37 for c in range(channels)]
    a = np.stack(planes, -1) + rng.normal(0, noise / 255.0, (height, width, channels))
    a = np.clip(a, 0, 1) * maximum
    return a.astype(np.uint16 if maximum > 255 else np.uint8)


def palette_of(entries, seed=5):
    return np.random.default_rng(seed).integers(0, 256, (entries, 3)).astype(np.uint8)


def far_match_png():
    """130 rows of 255 grey pixels (filter 0) in one hand-assembled fixed block: 32 768 literals, then a match of length 258 at distance
    32 768 and one of length 254 at the same distance"""
    rng = np.random.default_rng(11)
    rows = rng.integers(0, 256, (130, 256)).astype(np.uint8)
    rows[:, 0] = 0
    flat = rows.reshape(-1)
    flat[32768:32768 + 258] = flat[0:258]
    flat[33026:33280] = flat[258:512]
    w = fixed_block([int(v) for v in flat[:32768]] + [(258, 32768), (254, 32768)])
    return write_png(rows[:, 1:], 0, 8, raw_deflate=w.tobytes(), filtered=flat.tobytes())


def composite_png():
    """150x200 RGB: dynamic, (empty stored,) fixed, (empty stored,) stored, (empty stored,) dynamic"""
    img = photo(150, 200, seed=3)
    filtered = filter_rows(pack_rows(img, 8), 3, (4, 1, 2, 3, 0))
    cut = [0, 30000, 30900, 32000, len(filtered)]
    kws = [dict(), dict(strategy=zlib.Z_FIXED), dict(level=0), dict()]
    raw = composite_deflate([(filtered[a:b], kw) for a, b, kw in zip(cut[:-1], cut[1:], kws)])
    return write_png(img, 2, 8, raw_deflate=raw, filtered=filtered)


def format_cases():
    """name -> PNG bytes: every colour type / depth pair, the sub-byte ones at widths 13 and 16, every filter type in each"""
    out = {}
    rng = np.random.default_rng(21)
    for ct, depth in PAIRS:
        for W in ((13, 16) if depth < 8 else (13,)):
            H, ch, top = 9, CHANNELS[ct], (1 << depth) - 1
            if ct == 3:
                entries = min(1 << depth, 200)
                s = rng.integers(0, entries, (H, W, 1))
                pal, trns = palette_of(entries), (bytes([0, 128]) if depth == 4 else None)
            else:
                s = photo(H, W, ch, seed=ct * 31 + depth, maximum=top, noise=8.0) if depth >= 8 else rng.integers(0, top + 1, (H, W, ch))
                pal = trns = None
            out[f"fmt_ct{ct}_d{depth}_w{W}"] = write_png(s, ct, depth, filters=(0, 1, 2, 3, 4), palette=pal, trns=trns)
    return out


def device_cases():
    """name -> PNG bytes, the writer-made files the device tests run (all inside the default caps: tests/test_png_decode_model_cpu.py)"""
    out = {}
    out["many_blocks_48x64"] = write_png(photo(48, 64, seed=1), 2, 8, filters=(0, 1, 2, 3, 4), mem_level=1)
    out["composite_150x200"] = composite_png()
    out["constant_64x64"] = write_png(np.full((64, 64, 1), 77), 0, 8, filters=(0,))
    ramp = (np.arange(1024)[None, :] + np.zeros((96, 1), dtype=np.int64)) % 256
    out["ramp_96x1024"] = write_png(ramp[..., None], 0, 8, filters=(1,))
    out["far_match"] = far_match_png()
    for W in (1, 3, 200):
        out[f"paeth_130x{W}"] = write_png(photo(130, W, seed=7 + W), 2, 8, filters=(4,))
    out["one_pixel"] = write_png(np.array([[[9, 200, 31]]]), 2, 8, filters=(4,))
    out["run_broken_by_filter0"] = write_png(photo(70, 33, seed=9), 2, 8, filters=[4] * 20 + [0] + [3] * 30 + [1] + [2] * 18)
    out.update(format_cases())
    return out


def refusal_cases():
    """name -> (PNG bytes, name of the PngError subclass)"""
    img = photo(20, 24, seed=13)
    good = write_png(img, 2, 8, filters=(4,))
    h = parse(good)
    z = h["idat"]
    filtered = zlib.decompress(z)
    out = {}
    out["truncated_idat"] = (write_png(img, 2, 8, raw_deflate=z[2:len(z) // 2], filtered=filtered), "PngStream")
    out["adler_bit_flip"] = (write_png(img, 2, 8, filters=(4,), adler=zlib.adler32(filtered) ^ 0x100), "PngAdler")
    short = filter_rows(pack_rows(img[:-1], 8), 3, (4,))
    out["one_row_short"] = (write_png(img, 2, 8, filtered=short), "PngSize")
    out["adam7"] = (write_png(img, 2, 8, interlace=1), "PngInterlaced")
    out["fdict"] = (write_png(img, 2, 8, zlib_header=b"\x78\xbb"), "PngZlibHeader")
    far = fixed_block([0, 10, 20, (5, 9)]).tobytes()               # a match nine bytes back after three bytes of output
    out["distance_before_start"] = (write_png(np.zeros((1, 7, 1)), 0, 8, raw_deflate=far, filtered=bytes(8)), "PngDistance")
    out["filter_type_5"] = (write_png(img, 2, 8, filtered=bytes([5]) + filtered[1:]), "PngFilter")
    out["palette_index_past_plte"] = (write_png(np.full((3, 5, 1), 7), 3, 4, palette=palette_of(6)), "PngPalette")
    return out


def load_cases():
    """the committed fixture (tools/make_golden_png_decode.py): name -> (PNG bytes, the array PIL decoded from them)"""
    z = np.load(GOLDEN)
    return {k[:-4]: (z[k].tobytes(), z[k[:-4] + "_expect"]) for k in z.files if k.endswith("_png")}
