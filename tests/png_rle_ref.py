"""Slow model of the run-match coding of the device PNG encoder (csrc/png_rle.hip): a numpy tokenizer of its token rule, the token
histogram, a bit writer that assembles a deflate block from a token list and the table of pf_png_rle_build_table, and a numpy stand-in
for the four png_rle_* entry points of hip_ops in the manner of tests/png_fake_ops.py.  The length-symbol table is written out from
RFC 1951 3.2.5, not derived from the code under test.

Token rule: a run is a maximal stretch of equal bytes inside one row of the filtered stream (filter byte included).  Its first byte is a
literal; the other L - 1 bytes are cut into chunks of 258; a chunk of m >= 3 bytes is one match (length m, distance 1), a trailing
chunk of 1 or 2 bytes is literals.  A token is an int 0 .. 255 (literal) or a tuple (m,) (match)."""
import ctypes

import numpy as np
import torch

import patchfusion_amd._lib as L
from tests import png_ref as R
from tests.png_fake_ops import FakePngOps

NSYM, EOB, TABLE_WORDS, HIST_WORDS = 286, 256, 388, 546
HDR_BITS_WORD, DIST_WORD, LEN_WORD0, HDR_WORD0, HDR_BYTES = 286, 287, 288, 320, 272
HDR_BITS_BOUND = 3 + 14 + 57 + 287 * 7
MAX_BITS = 14
LENGTH_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LENGTH_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
EVERY_BASE = [3, 4, 10, 11, 18, 19, 34, 35, 66, 67, 130, 131, 257, 258]

# match length -> index of its length symbol (symbol 257 + k); 258 has a symbol of its own
_K = np.zeros(259, dtype=np.int64)
for _m in range(3, 259):
    _K[_m] = 28 if _m == 258 else max(k for k in range(28) if LENGTH_BASE[k] <= _m)


def length_symbol(m):
    """-> (symbol, extra bits, extra value)"""
    k = int(_K[m])
    return 257 + k, LENGTH_EXTRA[k], m - LENGTH_BASE[k]


def _runs(row):
    """heads and lengths of the runs of a 1-D uint8 array"""
    row = np.asarray(row, dtype=np.uint8)
    heads = np.concatenate([[0], np.flatnonzero(row[1:] != row[:-1]) + 1])
    return heads, np.diff(np.concatenate([heads, [len(row)]]))


def row_tokens(row):
    toks = []
    heads, lengths = _runs(row)
    for h, n in zip(heads.tolist(), lengths.tolist()):
        v = int(row[h])
        toks.append(v)
        rest = n - 1
        while rest > 0:
            m = min(258, rest)
            if m >= 3:
                toks.append((m,))
            else:
                toks += [v] * m
            rest -= m
    return toks


def tokens(rows):
    """rows: sequence of 1-D uint8 arrays (stream rows) -> the token list of all of them, runs never crossing a row"""
    out = []
    for row in rows:
        out += row_tokens(row)
    return out


def expand(toks):
    out = bytearray()
    for t in toks:
        if isinstance(t, tuple):
            out += bytes([out[-1]]) * t[0]
        else:
            out.append(t)
    return bytes(out)


def token_histogram(rows, nbands):
    """vectorised over the runs: -> (286 counts with [256] = nbands, total of extra bits)"""
    h = np.zeros(NSYM, dtype=np.int64)
    extra = 0
    for row in rows:
        row = np.asarray(row, dtype=np.uint8)
        heads, lengths = _runs(row)
        rest = lengths - 1
        tail = rest % 258
        np.add.at(h, row[heads].astype(np.int64), 1 + np.where(tail < 3, tail, 0))
        h[285] += int((rest // 258).sum())
        k = _K[tail[tail >= 3]]
        np.add.at(h, 257 + k, 1)
        extra += int(np.asarray(LENGTH_EXTRA)[k].sum())
    h[EOB] = nbands
    return h, extra


def histograms():
    """name -> 286 counts: the histograms of png_ref with length-symbol counts behind them"""
    out = {}
    for name, h in R.histograms().items():
        lens = np.array([1 + (k * 7919) % 53 for k in range(29)], dtype=np.uint32) * (1 if name != "flat" else 400)
        out[name] = np.concatenate([h, lens]).astype(np.uint32)
        out[name + "_no_matches"] = np.concatenate([h, np.zeros(29, dtype=np.uint32)]).astype(np.uint32)
    short = out["geometric"].copy()
    short[270:] = 0                                          # the header announces fewer than 286 codes
    out["geometric_short_lengths"] = short
    return out


def build_table(lib, hist):
    hist = np.ascontiguousarray(hist, dtype=np.uint32)
    assert hist.size == NSYM
    table = np.zeros(TABLE_WORDS, dtype=np.uint32)
    u32p = ctypes.POINTER(ctypes.c_uint32)
    rc = lib.pf_png_rle_build_table(hist.ctypes.data_as(u32p), table.ctypes.data_as(u32p))
    assert rc == 0, rc
    return table


def code_lengths(table):
    return [int(t) >> 16 for t in table[:NSYM]]


def put_block(w, table, toks):
    """header, tokens and end-of-block of one dynamic block, no flush"""
    hdr = table[HDR_WORD0:].tobytes()
    for i in range(int(table[HDR_BITS_WORD])):
        w.put((hdr[i >> 3] >> (i & 7)) & 1, 1)
    for t in list(toks) + [EOB]:
        if isinstance(t, tuple):
            s, nbits, value = length_symbol(t[0])
            assert int(table[LEN_WORD0 + s - 257]) == LENGTH_BASE[s - 257] | (LENGTH_EXTRA[s - 257] << 16)
        else:
            s = t
        c = int(table[s])
        assert c >> 16, f"symbol {s} has no code"
        w.put(c & 0xffff, c >> 16)
        if isinstance(t, tuple):
            w.put(value, nbits)
            d = int(table[DIST_WORD])
            w.put(d & 0xffff, d >> 16)


def deflate_with_table(table, toks):
    """one dynamic-Huffman block + the final empty stored block -> raw deflate bytes"""
    w = R.BitWriter()
    put_block(w, table, toks)
    w.put(1, 1)
    w.put(0, 2)
    w.align()
    return w.tobytes() + b"\x00\x00\xff\xff"


def run_row(lengths, values=(2, 4), separator=3):
    """residuals of one Sub-filtered u8c1 row: runs of the given lengths, values alternating, a separator byte between two runs; none
    of the default values is the filter byte of Sub, 1, so the first run starts at the first residual"""
    out = []
    for i, n in enumerate(lengths):
        if i:
            out.append(separator)
        out += [values[i % 2]] * n
    return np.array(out, dtype=np.uint8)


def image_of_residuals(res):
    """the u8c1 row whose Sub residuals are res"""
    return (np.cumsum(np.asarray(res, dtype=np.int64)) % 256).astype(np.uint8)


def run_length_cases():
    """name -> (u8c1 image [H, W], run lengths its filtered stream must show).  One row each unless said otherwise: with Sub, which
    the ramps these rows are make the cheapest filter, the stream is the filter byte 1 and the residuals below."""
    c = {}
    every = [1, 2, 3, 4, 258, 259, 260, 261, 262, 517, 518, 519, 520]
    c["every_length"] = (image_of_residuals(run_row(every))[None], every)
    c["run_to_the_last_byte"] = (image_of_residuals(run_row([5, 40]))[None], [40])
    c["run_from_the_filter_byte"] = (image_of_residuals(run_row([7, 3], values=(1, 2)))[None], [8])   # filter byte 1 + seven residuals 1
    across = run_row([1000, 100])                            # stream positions 1002 .. 1101 lie across the chunk boundary at 1024
    row = np.concatenate([across, np.full(1400 - len(across), 5, dtype=np.uint8)])
    row[len(across)] = 9
    c["across_the_chunk_boundary"] = (image_of_residuals(row)[None], [1000, 100])
    c["head_more_than_a_chunk_back"] = (image_of_residuals(run_row([49, 3000, 49]))[None], [3000])
    assert c["across_the_chunk_boundary"][0].shape == (1, 1400) and c["head_more_than_a_chunk_back"][0].shape == (1, 3100)
    c["every_length_ten_rows"] = (np.tile(image_of_residuals(run_row(every)), (10, 1)), every)  # rows 1 .. 9: Up, all zeros
    return c


def stream_run_lengths(stream, stride):
    out = []
    for r in range(len(stream) // stride):
        out += _runs(np.frombuffer(stream, dtype=np.uint8)[r * stride:(r + 1) * stride])[1].tolist()
    return out


class FakeRleOps(FakePngOps):
    """FakePngOps + the png_rle_* entry points: filters and streams from the parent, tokens from this module, the real table builder"""
    PNG_RLE_TABLE_WORDS, PNG_RLE_HIST_WORDS = TABLE_WORDS, HIST_WORDS

    def png_rle_workspace(self, image, bgr=False):
        H, W, ch, bits, _ = self.png_format(image, bgr)
        ws, out, nbands = self.png_workspace(image, bgr)
        return ws + 16 * nbands, out + 16 * nbands, nbands   # the header of this coding is 16 bytes longer

    def png_rle_filter_histogram(self, image, workspace, hist, bgr=False):
        lit = torch.zeros(257, dtype=torch.int32)
        self.png_filter_histogram(image, workspace, lit, bgr)
        nbands = (image.shape[0] + 7) // 8
        tok, extra = token_histogram(self.streams, nbands)
        h = np.zeros(HIST_WORDS, dtype=np.uint32)
        h[:257] = lit.numpy().view(np.uint32)
        h[257:257 + NSYM] = tok
        h[544], h[545] = extra & 0xffffffff, extra >> 32
        hist.copy_(torch.from_numpy(h.view(np.int32)))
        return hist

    @staticmethod
    def png_rle_build_table(hist):
        return build_table(L.load(), np.asarray(hist, dtype=np.int64).astype(np.uint32))

    def png_rle_encode(self, image, table, workspace, out, meta, bgr=False):
        H = image.shape[0]
        t = table.numpy().view(np.uint32)
        m, pos = [0, 0], 0
        for k in range((H + 7) // 8):
            rows = self.streams[8 * k:8 * k + 8]
            w = R.BitWriter()
            put_block(w, t, tokens(rows))
            w.put(0, 3)
            blob = w.tobytes() + b"\x00\x00\xff\xff"
            out[pos:pos + len(blob)] = torch.frombuffer(bytearray(blob), dtype=torch.uint8)
            pos += len(blob)
            d = np.concatenate(rows).astype(object)
            n = len(d)
            m += [len(blob), int(sum(d)) % 65521, int(sum((n - i) * int(v) for i, v in enumerate(d))) % 65521]
        m[0] = pos
        meta.copy_(torch.from_numpy(np.array(m, dtype=np.uint32).view(np.int32)))
        return out, meta
