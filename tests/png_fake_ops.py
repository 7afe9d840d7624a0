"""numpy stand-in for the PNG entry points of hip_ops (same arguments, same buffers, same band format), so that the host side of
postprocess.encode_png -- table hand-over, Adler-32 combination, zlib wrapper, chunks -- can be checked without a GPU.  Only the table
builder is the real one (it is host code).  Slow: small images only."""
import numpy as np
import torch

import patchfusion_amd._lib as L
from tests import png_ref as R


def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    return a if (pa <= pb and pa <= pc) else (b if pb <= pc else c)


class FakePngOps:
    PNG_BAND_ROWS, PNG_TABLE_WORDS = 8, 324

    @staticmethod
    def png_format(image, bgr=False):
        if image.dtype == torch.uint8 and image.dim() in (2, 3):
            return int(image.shape[0]), int(image.shape[1]), (1 if image.dim() == 2 else int(image.shape[2])), 8, int(bool(bgr))
        if image.dtype == torch.uint16 and image.dim() == 2:
            return int(image.shape[0]), int(image.shape[1]), 1, 16, int(bool(bgr))
        raise ValueError("png: unsupported image")

    def _rows(self, image, bgr):
        """[H][W * bpp] bytes in stream order"""
        a = image.numpy()
        if a.dtype == np.uint16:
            return a.astype(">u2").view(np.uint8).reshape(a.shape[0], -1)
        if bgr:
            a = a[..., [2, 1, 0] + list(range(3, a.shape[2]))]
        return np.ascontiguousarray(a).reshape(a.shape[0], -1)

    def png_workspace(self, image, bgr=False):
        H, W, ch, bits, _ = self.png_format(image, bgr)
        nbands = (H + 7) // 8
        slot = 256 + ((8 * (W * ch * bits // 8 + 1) + 1) * 15 + 7) // 8 + 8
        return H + nbands * slot, nbands * slot, nbands

    def png_filter_histogram(self, image, workspace, hist, bgr=False):
        H, W, ch, bits, _ = self.png_format(image, bgr)
        bpp = ch * bits // 8
        rows = self._rows(image, bgr).astype(np.int64)
        self.streams = []
        h = np.zeros(257, dtype=np.int64)
        for r in range(H):
            x = rows[r]
            a = np.concatenate([np.zeros(bpp, dtype=np.int64), x[:-bpp]]) if len(x) > bpp else np.zeros_like(x)
            b = rows[r - 1] if r else np.zeros_like(x)
            c = (np.concatenate([np.zeros(bpp, dtype=np.int64), b[:-bpp]]) if len(x) > bpp else np.zeros_like(x)) if r else np.zeros_like(x)
            pr = np.array([_paeth(int(p), int(q), int(s)) for p, q, s in zip(a, b, c)], dtype=np.int64)
            cands = {0: x % 256, 1: (x - a) % 256, 2: (x - b) % 256, 4: (x - pr) % 256}
            cost = {f: int(np.where(v < 128, v, 256 - v).sum()) for f, v in cands.items()}
            f = min((0, 1, 2, 4), key=lambda k: (cost[k], k))
            workspace[r] = f
            line = np.concatenate([[f], cands[f]]).astype(np.uint8)
            self.streams.append(line)
            h += np.bincount(line, minlength=257)
        h[256] = (H + 7) // 8
        hist.copy_(torch.from_numpy(h.astype(np.int32)))
        return hist

    @staticmethod
    def png_build_table(hist):
        return R.build_table(L.load(), np.asarray(hist, dtype=np.int64).astype(np.uint32))

    def png_encode(self, image, table, workspace, out, meta, bgr=False):
        H = image.shape[0]
        t = table.numpy().view(np.uint32)
        hdr = t[R.HDR_WORD0:].tobytes()
        m, pos = [0, 0], 0
        for k in range((H + 7) // 8):
            data = np.concatenate(self.streams[8 * k:8 * k + 8])
            w = R.BitWriter()
            for i in range(int(t[R.NSYM])):
                w.put((hdr[i >> 3] >> (i & 7)) & 1, 1)
            for s in list(data) + [R.EOB]:
                w.put(int(t[s]) & 0xffff, int(t[s]) >> 16)
            w.put(0, 3)
            blob = w.tobytes() + b"\x00\x00\xff\xff"
            out[pos:pos + len(blob)] = torch.frombuffer(bytearray(blob), dtype=torch.uint8)
            pos += len(blob)
            n = len(data)
            d = data.astype(object)
            m += [len(blob), int(sum(d)) % 65521, int(sum((n - i) * int(v) for i, v in enumerate(d))) % 65521]
        m[0] = pos
        meta.copy_(torch.from_numpy(np.array(m, dtype=np.uint32).view(np.int32)))
        return out, meta
