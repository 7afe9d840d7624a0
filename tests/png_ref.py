"""Slow, plain-Python side of the PNG encoder tests: the histograms the host table builder is tried on, a bit writer that assembles a
deflate block from the table it returns, and a PNG chunk reader.  Nothing here is fast or clever on purpose: it is the reference."""
import ctypes
import struct
import zlib

import numpy as np

NSYM, EOB, TABLE_WORDS, HDR_WORD0 = 257, 256, 324, 260


def histograms():
    """name -> 257 counts (uint32); [256] is the end-of-block"""
    h = {}
    h["flat"] = np.full(NSYM, 1000, dtype=np.uint32)
    one = np.zeros(NSYM, dtype=np.uint32)
    one[65], one[EOB] = 12345, 1
    h["one_literal"] = one
    two = np.zeros(NSYM, dtype=np.uint32)
    two[0], two[255], two[EOB] = 7, 900000, 3
    h["two_literals"] = two
    geo = np.zeros(NSYM, dtype=np.uint32)
    for s in range(28):
        geo[s * 9] = 1 << s
    geo[EOB] = 5
    h["geometric"] = geo
    fib = np.zeros(NSYM, dtype=np.uint32)
    a, b = 1, 1
    for s in range(40):                      # 40 Fibonacci weights: an unlimited Huffman tree is 39 deep
        fib[3 + s * 6] = a
        a, b = b, a + b
    fib[EOB] = 1
    h["fibonacci"] = fib
    return h


def build_table(lib, hist):
    """the C entry point through ctypes: numpy uint32 [324]"""
    hist = np.ascontiguousarray(hist, dtype=np.uint32)
    table = np.zeros(TABLE_WORDS, dtype=np.uint32)
    u32p = ctypes.POINTER(ctypes.c_uint32)
    rc = lib.pf_png_build_table(hist.ctypes.data_as(u32p), table.ctypes.data_as(u32p))
    assert rc == 0, rc
    return table


def code_lengths(table):
    return [int(t) >> 16 for t in table[:NSYM]]


class BitWriter:
    """deflate bit order: the first bit written is bit 0 of byte 0"""

    def __init__(self):
        self.bits = []

    def put(self, value, n):
        for b in range(n):
            self.bits.append((value >> b) & 1)

    def align(self):
        while len(self.bits) % 8:
            self.bits.append(0)

    def tobytes(self):
        self.align()
        out = bytearray(len(self.bits) // 8)
        for i, b in enumerate(self.bits):
            out[i >> 3] |= b << (i & 7)
        return bytes(out)


def deflate_with_table(table, data):
    """one dynamic-Huffman block of literals from the table's header and codes + the final empty stored block -> raw deflate bytes"""
    w = BitWriter()
    hdr = table[HDR_WORD0:].tobytes()
    for i in range(int(table[NSYM])):
        w.put((hdr[i >> 3] >> (i & 7)) & 1, 1)
    for s in list(data) + [EOB]:
        t = int(table[s])
        assert t >> 16, f"symbol {s} has no code"
        w.put(t & 0xffff, t >> 16)           # the table holds the codes bit-reversed, ready for this bit order
    w.put(1, 1)                              # BFINAL = 1, BTYPE = 0
    w.put(0, 2)
    w.align()
    return w.tobytes() + b"\x00\x00\xff\xff"


def png_chunks(png):
    """[(type, data)] of a PNG file, every CRC-32 checked"""
    assert png[:8] == b"\x89PNG\r\n\x1a\n"
    pos, out = 8, []
    while pos < len(png):
        n, kind = struct.unpack(">I4s", png[pos:pos + 8])
        data = png[pos + 8:pos + 8 + n]
        assert struct.unpack(">I", png[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(kind + data), kind
        out.append((kind, data))
        pos += 12 + n
    return out


def idat_payload(png):
    chunks = png_chunks(png)
    assert [k for k, _ in chunks] == [b"IHDR", b"IDAT", b"IEND"], [k for k, _ in chunks]
    return chunks[1][1]
