"""NumPy / pure-Python restatement of the progressive JPEG decoder (csrc/jpeg_host.h, csrc/jpeg_prog.hip): (a) a parser with the scan list,
a decoder of the four scan kinds to the coefficient array of tests/jpeg_ref.py (whose reconstruction turns it into pixels) and the model
of the subsequence rounds of the DC-first and AC-first device kernels; (b) a small progressive writer that emits any scan script from a
coefficient array, which PIL cannot.  tests/test_jpeg_prog_ref_cpu.py pins it against PIL.  Slow: small images only."""
import os

import numpy as np

from tests import jpeg_ref as R

ZIGZAG = [int(v) for v in R.ZIGZAG]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg_prog_cases.npz")
DC_FIRST, DC_REFINE, AC_FIRST, AC_REFINE = 0, 1, 2, 3
KINDS = ("dc_first", "dc_refine", "ac_first", "ac_refine")
CAP = 1 << 30                      # block counts saturate here, as on the device


def load_cases():
    """-> dict name -> (jpeg bytes, expected uint8 [H,W,3] or None for the files that must be refused)"""
    z = np.load(GOLDEN)
    names = sorted(k[5:] for k in z.files if k.startswith("jpeg_"))
    return {n: (z["jpeg_" + n].tobytes(), z["rgb_" + n] if "rgb_" + n in z.files else None) for n in names}


class Scan:
    def __repr__(self):
        return f"Scan({KINDS[self.kind]}, comps={self.comps}, {self.ss}-{self.se}, ah={self.ah}, al={self.al})"


def parse(data):
    """a progressive file -> (Header with the fields jpeg_ref.reconstruct reads, [Scan])"""
    h = R.Header()
    h.qt, h.orientation = {}, 1
    huff, dri, scans = {}, 0, []
    assert data[:2] == b"\xff\xd8"
    p = 2
    while True:
        assert data[p] == 0xff
        m = data[p + 1]
        if m == 0xd9:
            break
        n = (data[p + 2] << 8) | data[p + 3]
        q = data[p + 4:p + 2 + n]
        p += 2 + n
        if m == 0xdb:
            o = 0
            while o < len(q):
                t = np.zeros(64, dtype=np.int64)
                t[R.ZIGZAG] = np.frombuffer(q[o + 1:o + 65], dtype=np.uint8)
                h.qt[q[o] & 15] = t
                o += 65
        elif m == 0xc4:
            o = 0
            while o < len(q):
                bits = list(q[o + 1:o + 17])
                huff[(q[o] >> 4, q[o] & 15)] = (bits, list(q[o + 17:o + 17 + sum(bits)]))
                o += 17 + sum(bits)
        elif m == 0xc2:
            h.height, h.width, h.ncomp = (q[1] << 8) | q[2], (q[3] << 8) | q[4], q[5]
            h.comps = [(q[6 + 3 * c], q[7 + 3 * c] >> 4, q[7 + 3 * c] & 15, q[8 + 3 * c]) for c in range(h.ncomp)]
            h.samp = [(1, 1)] if h.ncomp == 1 else [(c[1], c[2]) for c in h.comps]
            h.hmax, h.vmax = h.samp[0]
            h.mcus_x, h.mcus_y = -(-h.width // (8 * h.hmax)), -(-h.height // (8 * h.vmax))
            h.comp_of = [c for c in range(h.ncomp) for _ in range(h.samp[c][0] * h.samp[c][1])]
            h.bpm = len(h.comp_of)
            h.nblocks = h.mcus_x * h.mcus_y * h.bpm
        elif m == 0xdd:
            dri = (q[0] << 8) | q[1]
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
            s = Scan()
            ns = q[0]
            ids = [c[0] for c in h.comps]
            s.comps = [ids.index(q[1 + 2 * c]) for c in range(ns)]
            s.tabs = [(q[2 + 2 * c] >> 4, q[2 + 2 * c] & 15) for c in range(ns)]
            s.ss, s.se, s.ah, s.al = q[1 + 2 * ns], q[2 + 2 * ns], q[3 + 2 * ns] >> 4, q[3 + 2 * ns] & 15
            s.kind = (DC_REFINE if s.ah else DC_FIRST) if s.ss == 0 else (AC_REFINE if s.ah else AC_FIRST)
            s.huff, s.dri, s.begin = dict(huff), dri, p
            if ns == 1:
                ch, cv = h.samp[s.comps[0]]
                s.bx, s.by = -(-(-(-h.width * ch // h.hmax)) // 8), -(-(-(-h.height * cv // h.vmax)) // 8)
                s.bpu, s.nblocks = 1, s.bx * s.by
            else:
                s.bpu, s.nblocks = h.bpm, h.nblocks
            while not (data[p] == 0xff and data[p + 1] != 0 and not 0xd0 <= data[p + 1] <= 0xd7):
                p += 1
            s.end = p
            scans.append(s)
    return h, scans


def block_map(h, s):
    """index in the coefficient array (MCU order) of every block of the scan's own walk"""
    if len(s.comps) > 1:
        return list(range(h.nblocks))
    c = s.comps[0]
    ch, cv = h.samp[c]
    first = h.comp_of.index(c)
    return [((by // cv) * h.mcus_x + bx // ch) * h.bpm + first + (by % cv) * ch + bx % ch for by in range(s.by) for bx in range(s.bx)]


def prepare_scan(data, s):
    out, segs, start, p = bytearray(), [], 0, s.begin
    while p < s.end:
        b = data[p]
        p += 1
        if b != 0xff:
            out.append(b)
            continue
        m = data[p]
        p += 1
        if m == 0:
            out.append(0xff)
        else:
            assert 0xd0 <= m <= 0xd7
            segs.append((start, 8 * len(out)))
            start = 8 * len(out)
    segs.append((start, 8 * len(out)))
    return bytes(out), segs


def seg_blocks(s, i):
    per = s.dri * s.bpu if s.dri else s.nblocks
    return min(per, s.nblocks - per * i)


def _extend(v, n):
    return v - (1 << n) + 1 if n and v < (1 << (n - 1)) else v


class LaneDecoder:
    """one decoder step of a DC-first scan (state b = block in the unit) or an AC-first scan (state k = zigzag position) exactly as the
    device kernels take it, EOB runs folded into the block count"""

    def __init__(self, h, s, scan):
        self.s = s
        bits = np.unpackbits(np.frombuffer(scan + b"\0" * 8, dtype=np.uint8)).astype(np.int64)
        self.bits = bits
        n = len(bits) - 16
        self.w16 = sum(bits[i:i + n] << (15 - i) for i in range(16)).tolist()
        if s.kind == DC_FIRST:
            self.tabs = [R.Huff(*s.huff[(0, t[0])]) for t in s.tabs]
            self.comp_of = h.comp_of if len(s.comps) > 1 else [0]
        else:
            self.tab = R.Huff(*s.huff[(1, s.tabs[0][1])])
        self.start = 0 if s.kind == DC_FIRST else s.ss

    def run(self, p, st, end, seg_end, sink=None, blk=0, limit=0):
        """decode while p < end -> (p, state, blocks completed, error bits); sink(blk, zigzag position, value) receives the coefficients"""
        s, w16, n, err = self.s, self.w16, 0, 0
        dc = s.kind == DC_FIRST
        while p < end:
            if sink and blk >= limit:
                break
            e = (self.tabs[self.comp_of[st]] if dc else self.tab).look[w16[p]]
            if not e:
                p += 1
                err |= 1
                continue
            ln, sym = e >> 8, e & 255
            r, sz = sym >> 4, sym & 15
            extra = sz if (dc or sz) else (r if r < 15 else 0)
            if p + ln + extra > seg_end:
                break
            v = w16[p + ln] >> (16 - extra) if extra else 0
            p += ln + extra
            if dc:
                if sink:
                    sink(blk, 0, _extend(v, sz))
                st = (st + 1) % s.bpu
                done = 1
            elif sz:
                st += r
                if st <= s.se:
                    if sink:
                        sink(blk, st, _extend(v, sz) * (1 << s.al))
                else:
                    err |= 8
                st += 1
                done = 1 if st > s.se else 0
            elif r == 15:
                st += 16
                done = 1 if st > s.se else 0
            else:
                done = (1 << r) + v
            if done:
                if not dc:
                    st = s.ss
                n, blk = min(n + done, CAP), min(blk + done, CAP)
                if sink and blk > limit:
                    err |= 4
                if sink and blk >= limit and seg_end - p > 7:
                    err |= 2
        return p, st, n, err


def decode_scan(h, s, data, coef):
    """one scan of any kind applied to coef (int64 [nblocks, 64], natural order)"""
    scan, segs = prepare_scan(data, s)
    bmap = block_map(h, s)
    per = s.dri * s.bpu if s.dri else s.nblocks
    if s.kind in (DC_FIRST, AC_FIRST):
        d = LaneDecoder(h, s, scan)
        diffs = np.zeros(s.nblocks, dtype=np.int64)

        def sink(blk, k, v):
            if s.kind == DC_FIRST:
                diffs[blk] = v
            else:
                coef[bmap[blk], ZIGZAG[k]] = v

        for i, (a, e) in enumerate(segs):
            first, nb = per * i, seg_blocks(s, i)
            p, st, n, err = d.run(a, d.start, e, e, sink, first, first + nb)
            assert not err and n == nb and st == d.start and 0 <= e - p <= 7, (s, i, err, n, nb)
            if s.kind == DC_FIRST:
                pred = [0] * len(s.comps)
                for j in range(first, first + nb):
                    c = d.comp_of[j % s.bpu]
                    pred[c] += int(diffs[j])
                    coef[bmap[j], 0] = pred[c] * (1 << s.al)
        return
    bits = np.unpackbits(np.frombuffer(scan + b"\0" * 8, dtype=np.uint8)).tolist()
    huff = R.Huff(*s.huff[(1, s.tabs[0][1])]) if s.kind == AC_REFINE else None
    p1 = 1 << s.al
    for i, (a, e) in enumerate(segs):
        p, eobrun = a, 0
        for j in range(per * i, per * i + seg_blocks(s, i)):
            blk = coef[bmap[j]]
            if s.kind == DC_REFINE:
                if bits[p]:
                    blk[0] |= p1
                p += 1
                continue
            k = s.ss

            def correct(k, p):
                if bits[p] and not (int(blk[ZIGZAG[k]]) & p1):
                    blk[ZIGZAG[k]] += p1 if blk[ZIGZAG[k]] >= 0 else -p1

            if eobrun == 0:
                while k <= s.se:
                    w = 0
                    for t in range(16):
                        w = (w << 1) | bits[p + t]
                    e16 = huff.look[w]
                    assert e16, "no such code"
                    p += e16 >> 8
                    r, sz = (e16 & 255) >> 4, e16 & 15
                    val = 0
                    if sz:
                        assert sz == 1
                        val = p1 if bits[p] else -p1
                        p += 1
                    elif r != 15:
                        eobrun = 1 << r
                        for t in range(r):
                            eobrun += bits[p + t] << (r - 1 - t)
                        p += r
                        break
                    while k <= s.se:
                        if blk[ZIGZAG[k]] != 0:
                            correct(k, p)
                            p += 1
                        else:
                            r -= 1
                            if r < 0:
                                break
                        k += 1
                    if val:
                        assert k <= s.se
                        blk[ZIGZAG[k]] = val
                    k += 1
            if eobrun > 0:
                while k <= s.se:
                    if blk[ZIGZAG[k]] != 0:
                        correct(k, p)
                        p += 1
                    k += 1
                eobrun -= 1
        assert eobrun == 0 and 0 <= e - p <= 7, (s, i, eobrun, e - p)


def decode_entropy(data, parsed=None, upto=None):
    """-> int16 [nblocks, 64] after every scan (or the first `upto` scans)"""
    h, scans = parsed or parse(data)
    coef = np.zeros((h.nblocks, 64), dtype=np.int64)
    for s in scans[:upto]:
        decode_scan(h, s, data, coef)
    return coef.astype(np.int16)


def decode(data, apply_orientation=True):
    h, scans = parse(data)
    return R.reconstruct(h, decode_entropy(data, (h, scans)), h.orientation if apply_orientation else 1)


def nonzero_masks(h, s, coef):
    """uint64 per block of the scan: bit k = the coefficient at zigzag position k is non-zero"""
    w = (1 << np.arange(64, dtype=np.uint64))
    return ((coef[block_map(h, s)][:, ZIGZAG] != 0).astype(np.uint64) * w).sum(axis=1, dtype=np.uint64)


def apply_records(h, s, coef, rec):
    """the host's refinement records [nblocks, 3] {correction, new, sign}, bits in zigzag order, applied to coef (any integer dtype) in place"""
    bmap, p1 = block_map(h, s), 1 << s.al
    bit = lambda m: ((m[:, None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)).astype(bool)      # noqa: E731
    corr, new, sign = bit(rec[:, 0]), bit(rec[:, 1]), bit(rec[:, 2])
    blk = coef[bmap][:, ZIGZAG].astype(np.int64)
    blk = np.where(corr, blk + np.where(blk >= 0, p1, -p1), blk)
    blk = np.where(new, np.where(sign, -p1, p1), blk)
    out = np.empty_like(blk)
    out[:, ZIGZAG] = blk
    coef[bmap] = out.astype(coef.dtype)


def sync_model(h, s, data, S, max_rounds=None):
    """the subsequence rounds of the device decoder of a DC-first or AC-first scan -> rounds run (jpeg_ref.sync_model's rules)"""
    scan, segs = prepare_scan(data, s)
    d = LaneDecoder(h, s, scan)
    lanes = []
    for a, e in segs:
        cnt = max(1, -(-(e - a) // S))
        lanes += [(a + i * S, min(a + i * S + S, e), e, i == 0) for i in range(cnt)]
    longest = max(max(1, -(-(e - a) // S)) for a, e in segs)
    cur = [d.run(st, d.start, en, se)[:3] for st, en, se, _ in lanes]
    entry = [(st, d.start) for st, en, se, _ in lanes]
    rounds = 0
    for r in range(1, longest):
        nxt = list(cur)
        for i in range(len(lanes)):
            if not lanes[i][3] and cur[i - 1][:2] != entry[i]:
                entry[i] = cur[i - 1][:2]
                nxt[i] = d.run(*entry[i], lanes[i][1], lanes[i][2])[:3]
        rounds = r
        changed = nxt != cur
        cur = nxt
        if not changed or r == max_rounds:
            break
    return rounds


# ------------------------------------------------------------------------------------------------ writer
PIL_SCRIPT = [((0, 1, 2), 0, 0, 0, 1), ((0,), 1, 5, 0, 2), ((2,), 1, 63, 0, 1), ((1,), 1, 63, 0, 1), ((0,), 6, 63, 0, 2), ((0,), 1, 63, 2, 1),
              ((0, 1, 2), 0, 0, 1, 0), ((2,), 1, 63, 1, 0), ((1,), 1, 63, 1, 0), ((0,), 1, 63, 1, 0)]


class _Tokens:
    """the symbols and raw bits of one scan; the Huffman table is made once they are all known"""

    def __init__(self):
        self.t = []

    def sym(self, table, s):
        self.t.append((table, s))

    def bits(self, v, n):
        if n:
            self.t.append((None, v & ((1 << n) - 1), n))

    def tables(self):
        used = {}
        for t in self.t:
            if t[0] is not None:
                used.setdefault(t[0], set()).add(t[1])
        out = {}
        for k, syms in used.items():
            syms = sorted(syms)
            L = max(1, len(syms).bit_length())            # every used symbol at one length L, n < 2^L: the all-ones code stays free
            out[k] = (L, syms, {s: i for i, s in enumerate(syms)})
        return out

    def emit(self, tables):
        acc = []
        for t in self.t:
            if t[0] is None:
                acc.append(format(t[1], f"0{t[2]}b"))
            else:
                L, _, code = tables[t[0]]
                acc.append(format(code[t[1]], f"0{L}b"))
        s = "".join(acc)
        s += "1" * (-len(s) % 8)
        raw = int(s, 2).to_bytes(len(s) // 8, "big") if s else b""
        return raw.replace(b"\xff", b"\xff\x00")


def _seg(marker, payload):
    return bytes([0xff, marker]) + (len(payload) + 2).to_bytes(2, "big") + payload


def write(h, coef, script):
    """frame header h (as parse gives it) + coefficient array [nblocks, 64] (natural order, MCU order) + scan script
    [(components, Ss, Se, Ah, Al)] -> the bytes of a progressive file.  Nothing is checked: an illegal script gives an illegal file."""
    coef = np.asarray(coef).astype(np.int64)
    out = bytearray(b"\xff\xd8" + _seg(0xe0, b"JFIF\0\x01\x01\0\0\x01\0\x01\0\0"))
    for t in sorted(h.qt):
        q = np.zeros(64, dtype=np.uint8)
        q[:] = h.qt[t][R.ZIGZAG]
        out += _seg(0xdb, bytes([t]) + q.tobytes())
    sof = bytes([8]) + h.height.to_bytes(2, "big") + h.width.to_bytes(2, "big") + bytes([h.ncomp])
    for cid, ch, cv, tq in h.comps:
        sof += bytes([cid, (ch << 4) | cv, tq])
    out += _seg(0xc2, sof)
    for comps, ss, se, ah, al in script:
        s = Scan()
        s.comps = list(comps)
        if len(comps) == 1 and comps[0] < h.ncomp:
            ch, cv = h.samp[comps[0]]
            s.bx, s.by = -(-(-(-h.width * ch // h.hmax)) // 8), -(-(-(-h.height * cv // h.vmax)) // 8)
            bmap, unit = block_map(h, s), [comps[0]]
        else:
            bmap, unit = list(range(h.nblocks)), [c for c in h.comp_of]        # an interleaved scan walks the whole array
            if len(comps) != h.ncomp:                                          # (an illegal script: the blocks of the named components only)
                bmap = [j for j in bmap if h.comp_of[j % h.bpm] in comps]
                unit = [c for c in h.comp_of if c in comps]
        tk = _Tokens()
        if ss == 0 and ah == 0:
            pred = {}
            for i, j in enumerate(bmap):
                c = unit[i % len(unit)]
                v = int(coef[j, 0]) >> al
                d = v - pred.get(c, 0)
                pred[c] = v
                n = abs(d).bit_length()
                tk.sym(("dc", c), n)
                tk.bits(d if d >= 0 else d - 1, n)
        elif ss == 0:
            for j in bmap:
                tk.bits((int(coef[j, 0]) >> al) & 1, 1)
        else:
            _write_ac(tk, coef, bmap, ss, se, ah, al)
        tabs = tk.tables()
        sos = bytes([len(comps)])
        for i, c in enumerate(comps):
            td = ta = 0
            if ("dc", c) in tabs:
                td = i
                L, syms, _ = tabs[("dc", c)]
                out += _seg(0xc4, bytes([td]) + bytes([len(syms) if l == L else 0 for l in range(1, 17)]) + bytes(syms))
            if "ac" in tabs:
                L, syms, _ = tabs["ac"]
                out += _seg(0xc4, bytes([0x10]) + bytes([len(syms) if l == L else 0 for l in range(1, 17)]) + bytes(syms))
            sos += bytes([h.comps[c][0] if c < h.ncomp else 99, (td << 4) | ta])
        out += _seg(0xda, sos + bytes([ss, se, (ah << 4) | al]))
        out += tk.emit(tabs)
    return bytes(out + b"\xff\xd9")


def _write_ac(tk, coef, bmap, ss, se, ah, al):
    """jcphuff.c's encode_mcu_AC_first / encode_mcu_AC_refine"""
    eobrun, held = 0, []                  # held: correction bits that follow the pending EOB run

    def flush():
        nonlocal eobrun, held
        if eobrun:
            n = eobrun.bit_length() - 1
            tk.sym("ac", n << 4)
            tk.bits(eobrun, n)
            eobrun = 0
        for b in held:
            tk.bits(b, 1)
        held = []

    for j in bmap:
        a = [abs(int(coef[j, ZIGZAG[k]])) >> al for k in range(64)]
        neg = [int(coef[j, ZIGZAG[k]]) < 0 for k in range(64)]
        r, br = 0, []
        if ah == 0:
            for k in range(ss, se + 1):
                if a[k] == 0:
                    r += 1
                    continue
                flush()
                while r > 15:
                    tk.sym("ac", 0xf0)
                    r -= 16
                n = a[k].bit_length()
                tk.sym("ac", (r << 4) | n)
                tk.bits(~a[k] if neg[k] else a[k], n)
                r = 0
        else:
            eob = max([k for k in range(ss, se + 1) if a[k] == 1], default=0)
            for k in range(ss, se + 1):
                if a[k] == 0:
                    r += 1
                    continue
                while r > 15 and k <= eob:
                    flush()
                    tk.sym("ac", 0xf0)
                    r -= 16
                    for b in br:
                        tk.bits(b, 1)
                    br = []
                if a[k] > 1:
                    br.append(a[k] & 1)
                    continue
                flush()
                tk.sym("ac", (r << 4) | 1)
                tk.bits(0 if neg[k] else 1, 1)
                for b in br:
                    tk.bits(b, 1)
                br, r = [], 0
        if r > 0 or br:
            eobrun += 1
            held += br
            if eobrun == 0x7fff:
                flush()
    flush()
