// Host side of the baseline JPEG decoder (csrc/jpeg.hip): marker parser, scan preparation, the sequential entropy decoder, the subsequence
// plan and the decode tables the device kernels read.  Like png_huff.h this header makes no GPU call and includes no GPU header, so a
// stand-alone program can include it (tests/host/jpeg_host_main.cpp runs it under the host sanitizers).
//
// Coefficient layout, shared by both entropy paths (this file's decode_entropy and jpeg.hip's kernels): int16 [nblocks][64], natural
// (de-zigzagged) order, NOT dequantised, blocks in MCU order and in scan order inside an MCU, DC absolute (predictor applied, int16 wrap).
#pragma once
#include <stdint.h>
#include <string.h>

#include "../../include/pf_hip.h"   // struct pf_jpeg_header and the PF_JPEG_E_* codes: plain C declarations, no GPU header

namespace pf_jpeg {

enum {
  OK = 0, E_ARG = 1, E_NOT_JPEG = PF_JPEG_E_NOT_JPEG, E_TRUNCATED = PF_JPEG_E_TRUNCATED, E_PROGRESSIVE = PF_JPEG_E_PROGRESSIVE,
  E_ARITHMETIC = PF_JPEG_E_ARITHMETIC, E_LOSSLESS = PF_JPEG_E_LOSSLESS, E_PRECISION = PF_JPEG_E_PRECISION, E_QUANT16 = PF_JPEG_E_QUANT16,
  E_COMPONENTS = PF_JPEG_E_COMPONENTS, E_COLORSPACE = PF_JPEG_E_COLORSPACE, E_SAMPLING = PF_JPEG_E_SAMPLING,
  E_MULTISCAN = PF_JPEG_E_MULTISCAN, E_DNL = PF_JPEG_E_DNL, E_MARKER = PF_JPEG_E_MARKER, E_RESTART = PF_JPEG_E_RESTART,
  E_NO_EOI = PF_JPEG_E_NO_EOI, E_TABLE = PF_JPEG_E_TABLE, E_STREAM = PF_JPEG_E_STREAM, E_SCAN = PF_JPEG_E_SCAN,
  NOT_CONVERGED = PF_JPEG_NOT_CONVERGED
};

static const uint8_t ZIGZAG[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                   41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                   30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

constexpr int SCAN_PAD = 64;                 // zero bytes after the unstuffed scan: every 64-bit window the decoders read lies inside
constexpr long MAX_SCAN_BYTES = 1l << 28;    // bit positions are 32-bit
constexpr int LOOK_BITS = 9;
// one decode table (device): look[1 << LOOK_BITS] uint16 (length << 8 | symbol, 0 = longer code), maxcode[18] int32 (by length, -1 = none),
// valoff[18] int32 (index of the first value of that length minus its first code), vals[256] bytes
constexpr int T_LOOK = 0, T_MAXCODE = (1 << LOOK_BITS) / 2, T_VALOFF = T_MAXCODE + 18, T_VALS = T_VALOFF + 18, T_WORDS = T_VALS + 64;
constexpr int TABLE_SLOTS = 6;               // [component][DC, AC]
constexpr int T_ZIGZAG = TABLE_SLOTS * T_WORDS;  // the zigzag table follows the six slots (64 bytes)
constexpr int TABLE_WORDS = T_ZIGZAG + 16;
static_assert(TABLE_WORDS == PF_JPEG_TABLE_WORDS, "pf_hip.h and jpeg_host.h disagree");

inline int rd16(const uint8_t* p) { return (p[0] << 8) | p[1]; }

// EXIF orientation out of an APP1 payload (after the length word); 1 when there is none
inline int exif_orientation(const uint8_t* p, int n) {
  if (n < 14 || memcmp(p, "Exif\0\0", 6)) return 1;
  const uint8_t* t = p + 6;
  const int tn = n - 6;
  bool le;
  if (t[0] == 'I' && t[1] == 'I') le = true;
  else if (t[0] == 'M' && t[1] == 'M') le = false;
  else return 1;
  auto u16 = [&](int o) { return le ? (t[o] | (t[o + 1] << 8)) : ((t[o] << 8) | t[o + 1]); };
  auto u32 = [&](int o) {
    return le ? ((uint32_t)t[o] | ((uint32_t)t[o + 1] << 8) | ((uint32_t)t[o + 2] << 16) | ((uint32_t)t[o + 3] << 24))
              : (((uint32_t)t[o] << 24) | ((uint32_t)t[o + 1] << 16) | ((uint32_t)t[o + 2] << 8) | (uint32_t)t[o + 3]);
  };
  if (u16(2) != 42) return 1;
  const uint32_t ifd = u32(4);
  if (ifd > (uint32_t)tn || tn - (int)ifd < 2) return 1;
  const int cnt = u16((int)ifd);
  for (int i = 0; i < cnt; ++i) {
    const long e = (long)ifd + 2 + 12l * i;
    if (e + 12 > tn) return 1;
    if (u16((int)e) == 0x0112) {
      if (u16((int)e + 2) != 3 || u32((int)e + 4) != 1) return 1;
      const int v = u16((int)e + 8);
      return (v >= 1 && v <= 8) ? v : 1;
    }
  }
  return 1;
}

// canonical code of one table: false when the lengths overflow the code space or count more than 256 values
inline bool huff_valid(const uint8_t* bits, const uint8_t* vals, bool dc) {
  int total = 0;
  uint32_t code = 0;
  for (int l = 1; l <= 16; ++l) {
    total += bits[l];
    code += bits[l];
    if (code > (1u << l)) return false;
    code <<= 1;
  }
  if (total > 256) return false;
  if (dc)
    for (int i = 0; i < total; ++i)
      if (vals[i] > 15) return false;
  return true;
}

// Marker parser: everything up to and including the SOS header.  Every refusal is a code of its own.
inline int parse(const uint8_t* d, long n, pf_jpeg_header* h) {
  if (!d || !h || n < 0) return E_ARG;
  memset(h, 0, sizeof(*h));
  h->orientation = 1;
  if (n < 4 || d[0] != 0xff || d[1] != 0xd8) return E_NOT_JPEG;
  long p = 2;
  bool jfif = false, adobe = false, sof_seen = false;
  int adobe_transform = -1;
  for (;;) {
    if (p + 2 > n) return E_TRUNCATED;
    if (d[p] != 0xff) return E_MARKER;
    while (p < n && d[p] == 0xff) ++p;          // fill bytes
    if (p >= n) return E_TRUNCATED;
    const int m = d[p++];
    if (m == 0xd8 || m == 0x01 || (m >= 0xd0 && m <= 0xd7)) continue;     // stand-alone markers
    if (m == 0xd9) return E_TRUNCATED;          // EOI before a scan
    if (p + 2 > n) return E_TRUNCATED;
    const int len = rd16(d + p);
    if (len < 2 || p + len > n) return E_TRUNCATED;
    const uint8_t* q = d + p + 2;
    const int ql = len - 2;
    p += len;
    if (m == 0xc2 || m == 0xc6) return E_PROGRESSIVE;
    if (m == 0xc3 || m == 0xc5 || m == 0xc7) return E_LOSSLESS;            // lossless and the differential (hierarchical) frames
    if (m >= 0xc9 && m <= 0xcf) return E_ARITHMETIC;                       // SOF9-15 and DAC (0xc4, DHT, is handled below)
    if (m == 0xdc) return E_DNL;
    if (m == 0xc0 || m == 0xc1) {
      if (sof_seen) return E_MARKER;
      if (ql < 6) return E_TRUNCATED;
      if (q[0] != 8) return E_PRECISION;
      h->height = rd16(q + 1);
      h->width = rd16(q + 3);
      h->ncomp = q[5];
      h->sof = m - 0xc0;
      if (h->height == 0) return E_DNL;
      if (h->width == 0) return E_ARG;
      if (h->ncomp != 1 && h->ncomp != 3) return E_COMPONENTS;
      if (ql < 6 + 3 * h->ncomp) return E_TRUNCATED;
      for (int c = 0; c < h->ncomp; ++c) {
        h->comp_id[c] = q[6 + 3 * c];
        h->comp_h[c] = q[7 + 3 * c] >> 4;
        h->comp_v[c] = q[7 + 3 * c] & 15;
        h->comp_tq[c] = q[8 + 3 * c];
        if (h->comp_h[c] < 1 || h->comp_h[c] > 4 || h->comp_v[c] < 1 || h->comp_v[c] > 4) return E_SAMPLING;
        if (h->comp_tq[c] > 3) return E_TABLE;
      }
      sof_seen = true;
    } else if (m == 0xdb) {
      int o = 0;
      while (o < ql) {
        const int pq = q[o] >> 4, tq = q[o] & 15;
        if (pq != 0) return pq == 1 ? E_QUANT16 : E_TABLE;
        if (tq > 3) return E_TABLE;
        if (o + 65 > ql) return E_TRUNCATED;
        for (int i = 0; i < 64; ++i) h->qt[tq][ZIGZAG[i]] = q[o + 1 + i];
        h->qt_present[tq] = 1;
        o += 65;
      }
    } else if (m == 0xc4) {
      int o = 0;
      while (o < ql) {
        const int tc = q[o] >> 4, th = q[o] & 15;
        if (tc > 1 || th > 3) return E_TABLE;
        if (o + 17 > ql) return E_TRUNCATED;
        const int t = tc * 4 + th;
        int total = 0;
        h->huff_bits[t][0] = 0;
        for (int l = 1; l <= 16; ++l) total += (h->huff_bits[t][l] = q[o + l]);
        if (total > 256) return E_TABLE;
        if (o + 17 + total > ql) return E_TRUNCATED;
        memset(h->huff_vals[t], 0, 256);
        memcpy(h->huff_vals[t], q + o + 17, (size_t)total);
        if (!huff_valid(h->huff_bits[t], h->huff_vals[t], tc == 0)) return E_TABLE;
        h->huff_present[t] = 1;
        o += 17 + total;
      }
    } else if (m == 0xdd) {
      if (ql < 2) return E_TRUNCATED;
      h->restart_interval = rd16(q);
    } else if (m == 0xe0) {
      if (ql >= 5 && !memcmp(q, "JFIF\0", 5)) jfif = true;
    } else if (m == 0xe1) {
      const int o = exif_orientation(q, ql);
      if (o != 1 || h->orientation == 1) h->orientation = o;
    } else if (m == 0xee) {
      if (ql >= 12 && !memcmp(q, "Adobe", 5)) {
        adobe = true;
        adobe_transform = q[11];
      }
    } else if (m == 0xda) {
      if (!sof_seen) return E_MARKER;
      if (ql < 1) return E_TRUNCATED;
      const int ns = q[0];
      if (ns < 1 || ns > 4 || ql < 1 + 2 * ns + 3) return E_TRUNCATED;
      if (ns != h->ncomp) return E_MULTISCAN;
      for (int c = 0; c < ns; ++c) {
        if (q[1 + 2 * c] != h->comp_id[c]) return E_SCAN;          // one interleaved scan, components in frame order
        h->comp_td[c] = q[2 + 2 * c] >> 4;
        h->comp_ta[c] = q[2 + 2 * c] & 15;
        if (h->comp_td[c] > 3 || h->comp_ta[c] > 3) return E_TABLE;
        if (!h->huff_present[h->comp_td[c]] || !h->huff_present[4 + h->comp_ta[c]] || !h->qt_present[h->comp_tq[c]]) return E_TABLE;
      }
      if (q[1 + 2 * ns] != 0 || q[2 + 2 * ns] != 63 || q[3 + 2 * ns] != 0) return E_SCAN;
      h->scan_begin = (int32_t)p;
      break;
    }
    // every other segment (APPn, COM, ...) is skipped
  }
  if (h->ncomp == 3) {
    // libjpeg's colour-space guess: JFIF -> YCbCr; Adobe -> its transform byte; else by component ids
    if (!jfif && adobe) {
      if (adobe_transform != 1) return E_COLORSPACE;
    } else if (!jfif && h->comp_id[0] == 'R' && h->comp_id[1] == 'G' && h->comp_id[2] == 'B') {
      return E_COLORSPACE;
    }
    if (h->comp_h[1] != 1 || h->comp_v[1] != 1 || h->comp_h[2] != 1 || h->comp_v[2] != 1) return E_SAMPLING;
    const int hv = h->comp_h[0] * 16 + h->comp_v[0];
    if (hv != 0x11 && hv != 0x21 && hv != 0x22) return E_SAMPLING;
  } else {
    h->comp_h[0] = h->comp_v[0] = 1;            // a single-component scan is not interleaved: one block per MCU whatever the frame says
  }
  h->hmax = h->comp_h[0];
  h->vmax = h->comp_v[0];
  h->mcus_x = (h->width + 8 * h->hmax - 1) / (8 * h->hmax);
  h->mcus_y = (h->height + 8 * h->vmax - 1) / (8 * h->vmax);
  h->blocks_per_mcu = 0;
  for (int c = 0; c < h->ncomp; ++c) h->blocks_per_mcu += h->comp_h[c] * h->comp_v[c];
  const long mcus = (long)h->mcus_x * h->mcus_y;
  h->nblocks = (int32_t)(mcus * h->blocks_per_mcu);
  h->nsegments = h->restart_interval ? (int32_t)((mcus + h->restart_interval - 1) / h->restart_interval) : 1;
  return OK;
}

// Scan preparation: `scan` (capacity >= len - scan_begin + SCAN_PAD + 4) receives the entropy-coded bytes with FF 00 -> FF and the RSTn
// markers removed, then >= SCAN_PAD zero bytes up to a multiple of 4; *scan_bytes = the size with the padding.  segs[2 * s] / [2 * s + 1]
// = first bit / end bit of restart interval s (nsegments pairs).
inline int prepare_scan(const uint8_t* d, long n, const pf_jpeg_header* h, uint8_t* scan, long cap, long* scan_bytes, uint32_t* segs) {
  if (!d || !h || !scan || !scan_bytes || !segs || h->scan_begin < 2 || h->scan_begin > n || h->nsegments < 1) return E_ARG;
  if (n - h->scan_begin > MAX_SCAN_BYTES || cap < n - h->scan_begin + SCAN_PAD + 4) return E_ARG;
  long o = 0, p = h->scan_begin;
  int seg = 0;
  segs[0] = 0;
  bool eoi = false;
  while (p < n) {
    const uint8_t b = d[p++];
    if (b != 0xff) {
      scan[o++] = b;
      continue;
    }
    while (p < n && d[p] == 0xff) ++p;          // fill bytes in front of a marker
    if (p >= n) break;
    const uint8_t m = d[p++];
    if (m == 0x00) {
      scan[o++] = 0xff;
    } else if (m >= 0xd0 && m <= 0xd7) {
      if (!h->restart_interval || (m - 0xd0) != (seg & 7) || seg + 1 >= h->nsegments) return E_RESTART;
      segs[2 * seg + 1] = (uint32_t)(o * 8);
      ++seg;
      segs[2 * seg] = (uint32_t)(o * 8);
    } else if (m == 0xd9) {
      eoi = true;
      break;
    } else if (m == 0xdc) {
      return E_DNL;
    } else if (m == 0xda) {
      return E_MULTISCAN;
    } else {
      return E_MARKER;
    }
  }
  if (!eoi) return E_NO_EOI;
  if (seg + 1 != h->nsegments) return E_RESTART;
  segs[2 * seg + 1] = (uint32_t)(o * 8);
  long total = (o + SCAN_PAD + 3) & ~3l;
  memset(scan + o, 0, (size_t)(total - o));
  *scan_bytes = total;
  return OK;
}

inline int seg_blocks(const pf_jpeg_header* h, int s) {   // blocks restart interval s holds
  if (!h->restart_interval) return h->nblocks;
  const long per = (long)h->restart_interval * h->blocks_per_mcu, left = (long)h->nblocks - per * s;
  return (int)(left < per ? left : per);
}

// component of block b of an MCU
inline void block_components(const pf_jpeg_header* h, int* comp) {
  int b = 0;
  for (int c = 0; c < h->ncomp; ++c)
    for (int i = 0; i < h->comp_h[c] * h->comp_v[c]; ++i) comp[b++] = c;
}

struct HostHuff {
  int32_t maxcode[18], valoff[18];
  const uint8_t* vals;
  void build(const uint8_t* bits, const uint8_t* v) {
    vals = v;
    int32_t code = 0, k = 0;
    for (int l = 1; l <= 16; ++l) {
      if (bits[l]) {
        valoff[l] = k - code;
        k += bits[l];
        code += bits[l];
        maxcode[l] = code - 1;
      } else {
        maxcode[l] = -1;
        valoff[l] = 0;
      }
      code <<= 1;
    }
    maxcode[0] = maxcode[17] = -1;
    valoff[0] = valoff[17] = 0;
  }
};

// Sequential entropy decoder: the second entropy path and the exact comparator of the device decoder.  coef: int16 [nblocks][64], written
// in full.  A bit reader that never leaves the segment: every read is checked against the segment's end bit.
inline int decode_entropy(const pf_jpeg_header* h, const uint8_t* scan, long scan_bytes, const uint32_t* segs, int16_t* coef) {
  if (!h || !scan || !segs || !coef || h->nblocks < 1 || h->blocks_per_mcu < 1 || h->blocks_per_mcu > 6) return E_ARG;
  HostHuff dc[3], ac[3];
  for (int c = 0; c < h->ncomp; ++c) {
    dc[c].build(h->huff_bits[h->comp_td[c]], h->huff_vals[h->comp_td[c]]);
    ac[c].build(h->huff_bits[4 + h->comp_ta[c]], h->huff_vals[4 + h->comp_ta[c]]);
  }
  int comp[6];
  block_components(h, comp);
  memset(coef, 0, (size_t)h->nblocks * 64 * sizeof(int16_t));
  const long per = h->restart_interval ? (long)h->restart_interval * h->blocks_per_mcu : 0;
  for (int s = 0; s < h->nsegments; ++s) {
    uint32_t p = segs[2 * s];
    const uint32_t end = segs[2 * s + 1];
    if (end < p || (long)(end >> 3) + SCAN_PAD > scan_bytes) return E_ARG;
    auto bit = [&](uint32_t at) { return (scan[at >> 3] >> (7 - (at & 7))) & 1; };
    auto symbol = [&](const HostHuff& t, int* sym) {
      int32_t code = 0;
      for (int l = 1; l <= 16; ++l) {
        if (p >= end) return false;
        code = (code << 1) | bit(p++);
        if (code <= t.maxcode[l]) {
          *sym = t.vals[(code + t.valoff[l]) & 255];
          return true;
        }
      }
      return false;
    };
    auto receive = [&](int n, int* v) {
      if (p + n > end) return false;
      int r = 0;
      for (int i = 0; i < n; ++i) r = (r << 1) | bit(p++);
      *v = n ? (r < (1 << (n - 1)) ? r - (1 << n) + 1 : r) : 0;
      return true;
    };
    int32_t pred[3] = {0, 0, 0};
    const long first = per * s;
    const int nb = seg_blocks(h, s);
    for (int i = 0; i < nb; ++i) {
      const int c = comp[i % h->blocks_per_mcu];
      int16_t* blk = coef + (first + i) * 64;
      int sym, v;
      if (!symbol(dc[c], &sym) || !receive(sym & 15, &v)) return E_STREAM;
      pred[c] += v;
      blk[0] = (int16_t)pred[c];
      int k = 1;
      while (k < 64) {
        if (!symbol(ac[c], &sym)) return E_STREAM;
        const int r = sym >> 4, n = sym & 15;
        if (n == 0) {
          if (r != 15) break;
          k += 16;
        } else {
          k += r;
          if (!receive(n, &v)) return E_STREAM;
          blk[ZIGZAG[k < 63 ? k : 63]] = (int16_t)v;      // libjpeg's clamp of an over-long run (its natural_order has 16 spare entries of 63)
          ++k;
        }
      }
    }
    if (end - p > 7) return E_STREAM;                       // at most the padding of the last byte may be left
  }
  return OK;
}

// Subsequence plan: every segment is cut into pieces of S bits (S % 32 == 0); a piece never straddles a segment; an empty segment still
// gets one (empty) lane so that its block count is checked.  lanes (null = count only): 3 words per lane {start bit, end bit, segment};
// segx: 4 words per segment {end bit, first lane, first block, block count}.  *longest = the most lanes any one segment has.
inline int plan(const pf_jpeg_header* h, const uint32_t* segs, int S, uint32_t* lanes, long lane_cap, uint32_t* segx, int* nlanes, int* longest) {
  if (!h || !segs || !nlanes || !longest || S < 32 || (S & 31) || S > (1 << 20) || h->nsegments < 1) return E_ARG;
  long nl = 0;
  int mx = 0;
  const long per = h->restart_interval ? (long)h->restart_interval * h->blocks_per_mcu : 0;
  for (int s = 0; s < h->nsegments; ++s) {
    const uint32_t a = segs[2 * s], e = segs[2 * s + 1];
    if (e < a) return E_ARG;
    long cnt = ((long)(e - a) + S - 1) / S;
    if (cnt < 1) cnt = 1;
    if (cnt > mx) mx = (int)cnt;
    if (lanes) {
      if (nl + cnt > lane_cap || !segx) return E_ARG;
      segx[4 * s] = e;
      segx[4 * s + 1] = (uint32_t)nl;
      segx[4 * s + 2] = (uint32_t)(per * s);
      segx[4 * s + 3] = (uint32_t)seg_blocks(h, s);
      for (long i = 0; i < cnt; ++i) {
        const long st = (long)a + i * S, en = st + S < (long)e ? st + S : (long)e;
        lanes[3 * (nl + i)] = (uint32_t)st;
        lanes[3 * (nl + i) + 1] = (uint32_t)en;
        lanes[3 * (nl + i) + 2] = (uint32_t)s;
      }
    }
    nl += cnt;
    if (nl > (1l << 30)) return E_ARG;
  }
  *nlanes = (int)nl;
  *longest = mx;
  return OK;
}

// The decode tables of the device kernels: slot 2 * c = DC table of component c, 2 * c + 1 = its AC table
inline int build_tables(const pf_jpeg_header* h, uint32_t* out) {
  if (!h || !out || h->ncomp < 1 || h->ncomp > 3) return E_ARG;
  memset(out, 0, TABLE_WORDS * sizeof(uint32_t));
  memcpy(out + T_ZIGZAG, ZIGZAG, 64);
  for (int c = 0; c < h->ncomp; ++c)
    for (int a = 0; a < 2; ++a) {
      const int t = a ? 4 + h->comp_ta[c] : h->comp_td[c];
      const uint8_t *bits = h->huff_bits[t], *vals = h->huff_vals[t];
      uint32_t* w = out + (2 * c + a) * T_WORDS;
      uint16_t* look = reinterpret_cast<uint16_t*>(w + T_LOOK);
      int32_t* maxcode = reinterpret_cast<int32_t*>(w + T_MAXCODE);
      int32_t* valoff = reinterpret_cast<int32_t*>(w + T_VALOFF);
      memcpy(w + T_VALS, vals, 256);
      int32_t code = 0, k = 0;
      for (int l = 0; l < 18; ++l) maxcode[l] = -1;
      for (int l = 1; l <= 16; ++l) {
        if (bits[l]) {
          valoff[l] = k - code;
          if (l <= LOOK_BITS)
            for (int i = 0; i < bits[l]; ++i) {
              const int first = (code + i) << (LOOK_BITS - l);
              for (int j = 0; j < (1 << (LOOK_BITS - l)); ++j) look[first + j] = (uint16_t)((l << 8) | vals[k + i]);
            }
          k += bits[l];
          code += bits[l];
          maxcode[l] = code - 1;
        }
        code <<= 1;
      }
    }
  return OK;
}

}  // namespace pf_jpeg
