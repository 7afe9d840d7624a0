"""numpy stand-in for the PNG-decode entry points of hip_ops (same arguments and buffers), built on tests/png_decode_ref.py, so that the
host side of preprocess.decode_png and ImagePreprocessor.read -- parse, chain walk with its rounds, fallbacks, status and Adler handling,
keyword routing -- can be checked without a GPU (the pattern of tests/jpeg_fake_ops.py).  Slow: small images only."""
import zlib

import numpy as np
import torch

from tests import png_decode_ref as R


def _header(h):
    return dict(width=h.width, height=h.height, depth=h.depth, color_type=h.color_type, channels=h.channels,
                palette=np.frombuffer(bytes(h.palette), dtype=np.uint8).reshape(256, 3))


class FakePngDecodeOps:
    def __init__(self, candidate_capacity=None):
        self.calls, self.candidate_capacity = [], candidate_capacity

    @staticmethod
    def _deflate(words, nbits):
        return words.numpy().view(np.uint8)[:nbits // 8].tobytes()

    def pngd_find(self, words, nbits, cand, count):
        found = R.find_candidates(self._deflate(words, nbits))
        cap = cand.numel() if self.candidate_capacity is None else min(cand.numel(), self.candidate_capacity)
        self.calls.append(("find", len(found)))
        count[0] = len(found) if len(found) <= cap else cand.numel() + 1        # an overflow counts past the capacity
        k = min(len(found), cap)
        cand[:k] = torch.tensor(found[:k], dtype=torch.int64).to(torch.int32)

    def pngd_scan(self, words, nbits, starts, n, max_block_bits, expected, records):
        b = R.Bits(self._deflate(words, nbits))
        self.calls.append(("scan", int(n), int(max_block_bits)))
        for i in range(n):
            start, end, out, st, final = R.scan(b, int(starts[i]) & 0xffffffff, max_block_bits, expected)
            records[i] = torch.tensor(np.array([start, end, out, st | final << 8], dtype=np.uint32).view(np.int32))
        return records

    def pngd_inflate(self, words, nbits, blocks, expected, lit, ref, status):
        table = [tuple(int(v) & 0xffffffff for v in row) for row in blocks.numpy()]
        self.calls.append(("inflate", len(table)))
        l, r, flags = R.inflate_blocks(self._deflate(words, nbits), table, expected)
        lit.copy_(torch.from_numpy(l))
        ref.copy_(torch.from_numpy(r.astype(np.int32)))
        status[0] |= flags

    def pngd_resolve(self, lit, ref, rounds, out):
        self.calls.append(("resolve", int(rounds)))
        r = ref.numpy().astype(np.int64)
        for _ in range(rounds):
            r = r[r]
        out.copy_(torch.from_numpy(lit.numpy()[r]))
        return out

    def pngd_adler(self, data, sums, result):
        self.calls.append(("adler", data.numel()))
        result[0] = int(np.array([zlib.adler32(data.numpy().tobytes())], dtype=np.uint32).view(np.int32)[0])

    def pngd_unfilter(self, header, inflated, recon, status):
        self.calls.append(("unfilter", header.bpp))
        raw = inflated.numpy().reshape(header.height, 1 + header.rowbytes).copy()
        if (raw[:, 0] > 4).any():
            status[0] |= 4
            raw[raw[:, 0] > 4, 0] = 0
        rows = R.unfilter(raw.tobytes(), header.height, header.rowbytes, header.bpp)
        recon.view(-1).view(torch.uint8).copy_(torch.from_numpy(rows.reshape(-1)))
        return recon

    def pngd_expand(self, header, recon, palette, image, status):
        self.calls.append(("expand", header.color_type, header.depth))
        h = _header(header)
        rows = recon.numpy().reshape(header.height, header.rowbytes)
        if header.color_type == 3:
            h["palette"] = palette.numpy().reshape(256, 3)
            idx = R.expand(rows, dict(h, color_type=0, depth=8 if header.depth == 8 else header.depth, palette=None))
            if header.depth < 8:
                idx = idx // (255 // ((1 << header.depth) - 1))
            if (idx >= header.plte_entries).any():
                status[0] |= 8
                idx = np.where(idx >= header.plte_entries, 0, idx)
            image.copy_(torch.from_numpy(h["palette"][idx]))
        else:
            image.copy_(torch.from_numpy(R.expand(rows, h)))
        return image

    def pngd_to_rgb8(self, image, rgb):
        self.calls.append(("to_rgb8", tuple(image.shape), str(image.dtype)))
        rgb.copy_(torch.from_numpy(R.to_rgb8(image.numpy())))
        return rgb

    # the two resizes ImagePreprocessor.__call__ runs: only recorded
    def u8_bicubic_to_f32(self, img, out, reverse_channels=False):
        self.calls.append(("bicubic", tuple(img.shape), img.numpy().copy()))
        out.zero_()

    def resize_bilinear_f32(self, src, dst):
        dst.zero_()
