// Host side of the JPEG decoders (csrc/jpeg.hip, and csrc/jpeg_prog.hip for progressive files): marker parsers, scan preparation, the
// sequential entropy decoders, the subsequence plan and the decode tables the device kernels read.  Like png_huff.h this header makes no GPU call and includes no GPU header, so a
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
  NOT_CONVERGED = PF_JPEG_NOT_CONVERGED,
  E_PROG_NO_FIRST = PF_JPEG_E_PROG_NO_FIRST, E_PROG_AH = PF_JPEG_E_PROG_AH, E_PROG_AL = PF_JPEG_E_PROG_AL,
  E_PROG_AC_COMPONENTS = PF_JPEG_E_PROG_AC_COMPONENTS, E_PROG_AC_BEFORE_DC = PF_JPEG_E_PROG_AC_BEFORE_DC, E_PROG_BAND = PF_JPEG_E_PROG_BAND,
  E_PROG_INCOMPLETE = PF_JPEG_E_PROG_INCOMPLETE, PROG_BASELINE = PF_JPEG_PROG_BASELINE,
  DC_FIRST = PF_JPEG_PROG_DC_FIRST, DC_REFINE = PF_JPEG_PROG_DC_REFINE, AC_FIRST = PF_JPEG_PROG_AC_FIRST, AC_REFINE = PF_JPEG_PROG_AC_REFINE
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

// the segment readers of the two parsers (parse below, prog_parse further down): q = the payload after the length word, ql = its size
inline int read_sof(const uint8_t* q, int ql, int m, bool sof_seen, pf_jpeg_header* h) {
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
  return OK;
}
inline int read_dqt(const uint8_t* q, int ql, pf_jpeg_header* h) {
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
  return OK;
}
inline int read_dht(const uint8_t* q, int ql, pf_jpeg_header* h) {
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
  return OK;
}
// colour space and sampling rules, then the frame's geometry (restart_interval must be set)
inline int finish_frame(pf_jpeg_header* h, bool jfif, bool adobe, int adobe_transform) {
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
      if (int rc = read_sof(q, ql, m, sof_seen, h)) return rc;
      sof_seen = true;
    } else if (m == 0xdb) {
      if (int rc = read_dqt(q, ql, h)) return rc;
    } else if (m == 0xc4) {
      if (int rc = read_dht(q, ql, h)) return rc;
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
  return finish_frame(h, jfif, adobe, adobe_transform);
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

// one decode table of the device kernels (T_WORDS words at w, zeroed by the caller) from a DHT table
inline void build_table_slot(const uint8_t* bits, const uint8_t* vals, uint32_t* w) {
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

// The decode tables of the device kernels: slot 2 * c = DC table of component c, 2 * c + 1 = its AC table
inline int build_tables(const pf_jpeg_header* h, uint32_t* out) {
  if (!h || !out || h->ncomp < 1 || h->ncomp > 3) return E_ARG;
  memset(out, 0, TABLE_WORDS * sizeof(uint32_t));
  memcpy(out + T_ZIGZAG, ZIGZAG, 64);
  for (int c = 0; c < h->ncomp; ++c)
    for (int a = 0; a < 2; ++a) {
      const int t = a ? 4 + h->comp_ta[c] : h->comp_td[c];
      build_table_slot(h->huff_bits[t], h->huff_vals[t], out + (2 * c + a) * T_WORDS);
    }
  return OK;
}


// ------------------------------------------------------------------------------------------------ progressive files (opt-in)
// The host side of csrc/jpeg_prog.hip: the parser with libjpeg's progression bookkeeping, scan preparation, the sequential decoder of
// all four scan kinds (jdphuff.c) and the stand-alone AC-refinement decoder.  Every bit read is checked against its segment's end bit,
// every block index against the scan's block count, every zigzag position against the band: an error or a decode, never a wild access.

constexpr int MAX_AL = 13;                   // libjpeg's limit on the successive-approximation shift

// Parser of a whole progressive file -> frame header + scan list.  PROG_BASELINE as soon as a baseline frame header shows.
inline int prog_parse(const uint8_t* d, long n, pf_jpeg_header* h, pf_jpeg_prog_scan* scans, int cap, int* nscans) {
  if (!d || !h || !scans || !nscans || n < 0 || cap < 0) return E_ARG;
  memset(h, 0, sizeof(*h));
  h->orientation = 1;
  *nscans = 0;
  if (n < 4 || d[0] != 0xff || d[1] != 0xd8) return E_NOT_JPEG;
  if (n > MAX_SCAN_BYTES) return E_ARG;
  long p = 2;
  bool jfif = false, adobe = false, sof_seen = false, eoi = false;
  int adobe_transform = -1, restart = 0;
  int8_t coef_bits[3][64];                     // libjpeg's coef_bits: -1 = not sent yet, else the Al it was last sent at
  memset(coef_bits, -1, sizeof(coef_bits));
  while (!eoi) {
    if (p + 2 > n) return *nscans ? E_NO_EOI : E_TRUNCATED;
    if (d[p] != 0xff) return E_MARKER;
    while (p < n && d[p] == 0xff) ++p;          // fill bytes
    if (p >= n) return *nscans ? E_NO_EOI : E_TRUNCATED;
    const int m = d[p++];
    if (m == 0xd8 || m == 0x01) continue;
    if (m >= 0xd0 && m <= 0xd7) {
      if (*nscans) return E_RESTART;            // an RSTn after a scan's data would have been taken with that scan
      continue;
    }
    if (m == 0xd9) {
      if (!*nscans) return E_TRUNCATED;         // EOI before a scan
      eoi = true;
      break;
    }
    if (p + 2 > n) return E_TRUNCATED;
    const int len = rd16(d + p);
    if (len < 2 || p + len > n) return E_TRUNCATED;
    const uint8_t* q = d + p + 2;
    const int ql = len - 2;
    p += len;
    if (m == 0xc0 || m == 0xc1) return PROG_BASELINE;
    if (m == 0xc6) return E_PROGRESSIVE;                                   // differential progressive (hierarchical)
    if (m == 0xc3 || m == 0xc5 || m == 0xc7) return E_LOSSLESS;
    if (m >= 0xc9 && m <= 0xcf) return E_ARITHMETIC;                       // SOF10, progressive arithmetic, among them
    if (m == 0xdc) return E_DNL;
    if (m == 0xc2) {
      if (int rc = read_sof(q, ql, m, sof_seen, h)) return rc;
      sof_seen = true;
      if (int rc = finish_frame(h, true, false, -1)) return rc;            // geometry now (scans need it); the colour guess waits for the end
    } else if (m == 0xdb) {
      if (int rc = read_dqt(q, ql, h)) return rc;
    } else if (m == 0xc4) {
      if (int rc = read_dht(q, ql, h)) return rc;
    } else if (m == 0xdd) {
      if (ql < 2) return E_TRUNCATED;
      restart = rd16(q);
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
      if (*nscans >= cap) return E_ARG;
      if (ql < 1) return E_TRUNCATED;
      const int ns = q[0];
      if (ns < 1 || ns > 4 || ql < 1 + 2 * ns + 3) return E_TRUNCATED;
      pf_jpeg_prog_scan* sc = scans + *nscans;
      memset(sc, 0, sizeof(*sc));
      sc->ncomp = ns;
      sc->ss = q[1 + 2 * ns];
      sc->se = q[2 + 2 * ns];
      sc->ah = q[3 + 2 * ns] >> 4;
      sc->al = q[3 + 2 * ns] & 15;
      if (sc->ss > sc->se || sc->se > 63 || (sc->ss == 0 && sc->se != 0)) return E_PROG_BAND;
      if (sc->ss > 0 && ns != 1) return E_PROG_AC_COMPONENTS;
      if (ns != 1 && ns != h->ncomp) return E_SCAN;                        // interleaved: every component, in frame order
      for (int c = 0; c < ns; ++c) {
        int f = -1;
        if (ns == 1) {
          for (int i = 0; i < h->ncomp; ++i)
            if (q[1] == h->comp_id[i]) { f = i; break; }
        } else if (q[1 + 2 * c] == h->comp_id[c]) {
          f = c;
        }
        if (f < 0) return E_SCAN;
        sc->comp[c] = f;
        sc->td[c] = q[2 + 2 * c] >> 4;
        sc->ta[c] = q[2 + 2 * c] & 15;
        if (sc->td[c] > 3 || sc->ta[c] > 3) return E_TABLE;
      }
      if (sc->al > MAX_AL) return E_SCAN;
      if (sc->ah && sc->al != sc->ah - 1) return E_PROG_AL;
      sc->kind = sc->ss == 0 ? (sc->ah ? DC_REFINE : DC_FIRST) : (sc->ah ? AC_REFINE : AC_FIRST);
      for (int c = 0; c < ns; ++c) {
        if (sc->kind == DC_FIRST && !h->huff_present[sc->td[c]]) return E_TABLE;
        if (sc->ss > 0 && !h->huff_present[4 + sc->ta[c]]) return E_TABLE;
        int8_t* cb = coef_bits[sc->comp[c]];
        if (sc->ss > 0 && cb[0] < 0) return E_PROG_AC_BEFORE_DC;
        for (int k = sc->ss; k <= sc->se; ++k) {
          if (cb[k] < 0 && sc->ah) return E_PROG_NO_FIRST;
          if (cb[k] >= 0 && sc->ah != cb[k]) return E_PROG_AH;             // with Ah = 0: a first scan that comes twice
          if (cb[k] >= 0 && !sc->ah) return E_PROG_AH;
          cb[k] = (int8_t)sc->al;
        }
      }
      memcpy(sc->huff_bits, h->huff_bits, sizeof(sc->huff_bits));
      memcpy(sc->huff_vals, h->huff_vals, sizeof(sc->huff_vals));
      sc->restart_interval = restart;
      long units;
      if (ns == 1) {
        const int f = sc->comp[0];
        sc->blocks_x = ((h->width * h->comp_h[f] + h->hmax - 1) / h->hmax + 7) / 8;
        sc->blocks_y = ((h->height * h->comp_v[f] + h->vmax - 1) / h->vmax + 7) / 8;
        sc->blocks_per_unit = 1;
        units = (long)sc->blocks_x * sc->blocks_y;
      } else {
        sc->blocks_per_unit = h->blocks_per_mcu;
        units = (long)h->mcus_x * h->mcus_y;
      }
      sc->nblocks = (int32_t)(units * sc->blocks_per_unit);
      sc->nsegments = restart ? (int32_t)((units + restart - 1) / restart) : 1;
      sc->begin = (int32_t)p;
      // the entropy-coded data runs to the next marker that is neither a stuffed FF 00 nor RSTn
      for (;;) {
        if (p >= n) return E_NO_EOI;
        if (d[p] != 0xff) { ++p; continue; }
        long t = p;
        while (t < n && d[t] == 0xff) ++t;
        if (t >= n) return E_NO_EOI;
        if (d[t] == 0 || (d[t] >= 0xd0 && d[t] <= 0xd7)) { p = t + 1; continue; }
        break;
      }
      sc->end = (int32_t)p;
      ++*nscans;
    }
    // every other segment (APPn, COM, ...) is skipped
  }
  if (!sof_seen) return E_MARKER;
  h->restart_interval = 0;
  if (int rc = finish_frame(h, jfif, adobe, adobe_transform)) return rc;
  for (int c = 0; c < h->ncomp; ++c) {
    if (!h->qt_present[h->comp_tq[c]]) return E_TABLE;
    for (int k = 0; k < 64; ++k)
      if (coef_bits[c][k] != 0) return E_PROG_INCOMPLETE;
  }
  return OK;
}

inline bool prog_scan_ok(const pf_jpeg_prog_scan* sc) {
  if (!sc || sc->kind < DC_FIRST || sc->kind > AC_REFINE || sc->ncomp < 1 || sc->ncomp > 3 || sc->nblocks < 1 || sc->nsegments < 1) return false;
  if (sc->ss < 0 || sc->ss > sc->se || sc->se > 63 || sc->al < 0 || sc->al > MAX_AL || sc->restart_interval < 0) return false;
  if ((sc->kind <= DC_REFINE) != (sc->ss == 0) || (sc->ss == 0 && sc->se != 0) || (sc->ss > 0 && sc->ncomp != 1)) return false;
  if (sc->blocks_per_unit < 1 || sc->blocks_per_unit > 6 || sc->nblocks % sc->blocks_per_unit) return false;
  if (sc->ncomp == 1 && (sc->blocks_per_unit != 1 || sc->blocks_x < 1 || sc->blocks_y < 1 || (long)sc->blocks_x * sc->blocks_y != sc->nblocks)) return false;
  const long units = sc->nblocks / sc->blocks_per_unit;
  if (sc->nsegments != (sc->restart_interval ? (units + sc->restart_interval - 1) / sc->restart_interval : 1)) return false;
  for (int c = 0; c < sc->ncomp; ++c)
    if (sc->comp[c] < 0 || sc->comp[c] > 2 || sc->td[c] < 0 || sc->td[c] > 3 || sc->ta[c] < 0 || sc->ta[c] > 3) return false;
  return sc->begin >= 2 && sc->end >= sc->begin;
}

// does the scan walk this frame?  (the pair the device entry points and the host decoder are handed)
inline bool prog_scan_fits(const pf_jpeg_header* h, const pf_jpeg_prog_scan* sc) {
  if (!h || !prog_scan_ok(sc) || h->nblocks < 1 || h->blocks_per_mcu < 1 || h->blocks_per_mcu > 6 || h->mcus_x < 1) return false;
  if (sc->ncomp > 1) return sc->ncomp == h->ncomp && sc->blocks_per_unit == h->blocks_per_mcu && sc->nblocks == h->nblocks;
  const int f = sc->comp[0];
  if (f >= h->ncomp || h->comp_h[f] < 1 || h->comp_v[f] < 1) return false;
  const long mcus_y = h->nblocks / h->blocks_per_mcu / h->mcus_x;
  return sc->blocks_x <= h->mcus_x * h->comp_h[f] && sc->blocks_y <= mcus_y * h->comp_v[f];
}

inline int prog_seg_blocks(const pf_jpeg_prog_scan* sc, int s) {
  if (!sc->restart_interval) return sc->nblocks;
  const long per = (long)sc->restart_interval * sc->blocks_per_unit, left = (long)sc->nblocks - per * s;
  return (int)(left < per ? left : per);
}

// index in the coefficient array (MCU order) of block j of the scan's own walk
inline long prog_block_index(const pf_jpeg_header* h, const pf_jpeg_prog_scan* sc, long j) {
  if (sc->ncomp > 1) return j;
  const int f = sc->comp[0];
  int first = 0;
  for (int c = 0; c < f; ++c) first += h->comp_h[c] * h->comp_v[c];
  const int bx = (int)(j % sc->blocks_x), by = (int)(j / sc->blocks_x), ch = h->comp_h[f], cv = h->comp_v[f];
  return ((long)(by / cv) * h->mcus_x + bx / ch) * h->blocks_per_mcu + first + (by % cv) * ch + bx % ch;
}

inline int prog_block_map(const pf_jpeg_header* h, const pf_jpeg_prog_scan* sc, int32_t* map) {
  if (!map || !prog_scan_fits(h, sc)) return E_ARG;
  for (long j = 0; j < sc->nblocks; ++j) map[j] = (int32_t)prog_block_index(h, sc, j);
  return OK;
}

// Scan preparation of one scan: as prepare_scan, over the byte range the parser found (it holds data, stuffed FFs, fill bytes and RSTn only)
inline int prog_prepare_scan(const uint8_t* d, long n, const pf_jpeg_prog_scan* sc, uint8_t* scan, long cap, long* scan_bytes, uint32_t* segs) {
  if (!d || !scan || !scan_bytes || !segs || !prog_scan_ok(sc) || sc->end > n) return E_ARG;
  if (sc->end - sc->begin > MAX_SCAN_BYTES || cap < sc->end - sc->begin + SCAN_PAD + 4) return E_ARG;
  long o = 0, p = sc->begin;
  int seg = 0;
  segs[0] = 0;
  while (p < sc->end) {
    const uint8_t b = d[p++];
    if (b != 0xff) {
      scan[o++] = b;
      continue;
    }
    while (p < sc->end && d[p] == 0xff) ++p;
    if (p >= sc->end) return E_MARKER;
    const uint8_t m = d[p++];
    if (m == 0x00) {
      scan[o++] = 0xff;
    } else if (m >= 0xd0 && m <= 0xd7) {
      if (!sc->restart_interval || (m - 0xd0) != (seg & 7) || seg + 1 >= sc->nsegments) return E_RESTART;
      segs[2 * seg + 1] = (uint32_t)(o * 8);
      ++seg;
      segs[2 * seg] = (uint32_t)(o * 8);
    } else {
      return E_MARKER;
    }
  }
  if (seg + 1 != sc->nsegments) return E_RESTART;
  segs[2 * seg + 1] = (uint32_t)(o * 8);
  const long total = (o + SCAN_PAD + 3) & ~3l;
  memset(scan + o, 0, (size_t)(total - o));
  *scan_bytes = total;
  if (sc->kind == DC_REFINE)                     // one raw bit per block: checked here, so that the device kernel needs no error word
    for (int s = 0; s < sc->nsegments; ++s) {
      const long bits = (long)segs[2 * s + 1] - segs[2 * s], nb = prog_seg_blocks(sc, s);
      if (bits < nb || bits - nb > 7) return E_STREAM;
    }
  return OK;
}

// a bit reader that never leaves [p, end)
struct ProgBits {
  const uint8_t* scan;
  uint32_t p, end;
  bool bit(int* b) {
    if (p >= end) return false;
    *b = (scan[p >> 3] >> (7 - (p & 7))) & 1;
    ++p;
    return true;
  }
  bool bits(int n, int* v) {                     // n raw bits, 0 <= n <= 16
    if ((long)p + n > end) return false;
    int r = 0, b = 0;
    for (int i = 0; i < n; ++i) {
      bit(&b);
      r = (r << 1) | b;
    }
    *v = r;
    return true;
  }
  bool symbol(const HostHuff& t, int* sym) {
    int32_t code = 0;
    int b = 0;
    for (int l = 1; l <= 16; ++l) {
      if (!bit(&b)) return false;
      code = (code << 1) | b;
      if (code <= t.maxcode[l]) {
        *sym = t.vals[(code + t.valoff[l]) & 255];
        return true;
      }
    }
    return false;
  }
};
inline int huff_extend(int r, int s) { return s ? (r < (1 << (s - 1)) ? r - (1 << s) + 1 : r) : 0; }

// the host's fast bit reader and table for AC refinement, which stays on the host in the device path: a 57-bit window and a
// LOOK_BITS-bit first-level table, as the device kernels have
struct FastHuff : HostHuff {
  uint16_t look[1 << LOOK_BITS];               // length << 8 | symbol, 0 = a longer code
  void build(const uint8_t* bits, const uint8_t* v) {
    HostHuff::build(bits, v);
    memset(look, 0, sizeof(look));
    int32_t code = 0, k = 0;
    for (int l = 1; l <= 16; ++l) {
      if (l <= LOOK_BITS)
        for (int i = 0; i < bits[l]; ++i) {
          const int first = (code + i) << (LOOK_BITS - l);
          for (int j = 0; j < (1 << (LOOK_BITS - l)); ++j) look[first + j] = (uint16_t)((l << 8) | v[k + i]);
        }
      k += bits[l];
      code += bits[l];
      code <<= 1;
    }
  }
};
struct FastBits {
  const uint8_t* scan;                         // padded by SCAN_PAD zero bytes: the eight bytes at any p <= end lie inside
  uint32_t p, end;
  uint64_t buf;                                // the bits from p on, left-aligned; cnt of them are valid (start with cnt = 0)
  int cnt;
  void need(int n) {                           // n <= 57
    if (cnt >= n) return;
    uint64_t w;
    memcpy(&w, scan + (p >> 3), 8);
    buf = __builtin_bswap64(w) << (p & 7);
    cnt = 64 - (int)(p & 7);
  }
  void drop(int n) {
    buf <<= n;
    cnt -= n;
    p += (uint32_t)n;
  }
  bool take(int n, uint32_t* v) {              // n raw bits, 0 <= n <= 16
    if ((long)p + n > end) return false;
    *v = 0;
    if (n) {
      need(n);
      *v = (uint32_t)(buf >> (64 - n));
      drop(n);
    }
    return true;
  }
  bool symbol(const FastHuff& t, int* sym) {
    need(16);
    const uint32_t e = t.look[buf >> (64 - LOOK_BITS)];
    int len = (int)(e >> 8);
    *sym = (int)(e & 255u);
    if (!e)
      for (int l = LOOK_BITS + 1; l <= 16; ++l) {
        const int32_t code = (int32_t)(buf >> (64 - l));
        if (code <= t.maxcode[l]) {
          len = l;
          *sym = t.vals[(code + t.valoff[l]) & 255];
          break;
        }
      }
    if (!len || (long)p + len > end) return false;
    drop(len);
    return true;
  }
  // one correction bit for every set bit of m, lowest first; the bits that are 1 are added to *corr
  bool corrections(uint64_t m, uint64_t* corr) {
    if ((long)p + __builtin_popcountll(m) > end) return false;
    for (; m; m &= m - 1) {
      need(1);
      if (buf >> 63) *corr |= m & (~m + 1);
      drop(1);
    }
    return true;
  }
};

// AC refinement of one scan (jdphuff.c decode_mcu_AC_refine) against the non-zero masks of the blocks: bit k = the coefficient at zigzag
// position k is non-zero.  nonzero(j) gives the mask of the scan's block j; update(j, correction, fresh, sign) receives what the scan does
// to it, in the same bit order: `correction` coefficients move away from zero by 1 << Al, `fresh` ones (zero so far) become +-(1 << Al),
// minus where `sign` is set.  The coefficient values are not needed: in an accepted progression every non-zero coefficient of the band is
// a multiple of 2 << Al, so libjpeg's test of the bit being refined never fails.  libjpeg walks the band coefficient by coefficient; here
// a symbol's run is the (r + 1)-th zero bit of the mask from k on and the correction bits are those of the set bits passed on the way,
// which is the same walk.  A new coefficient past the band's end or of a size other than 1: E_STREAM.
template <class Nonzero, class Update>
inline int prog_refine_ac_core(const pf_jpeg_prog_scan* sc, const uint8_t* scan, long scan_bytes, const uint32_t* segs, Nonzero nonzero, Update update) {
  if (!prog_scan_ok(sc) || sc->kind != AC_REFINE || !scan || !segs) return E_ARG;
  FastHuff ac;
  ac.build(sc->huff_bits[4 + sc->ta[0]], sc->huff_vals[4 + sc->ta[0]]);
  const long per = sc->restart_interval ? (long)sc->restart_interval : 0;
  const uint64_t upto_se = sc->se == 63 ? ~0ull : (1ull << (sc->se + 1)) - 1;
  for (int s = 0; s < sc->nsegments; ++s) {
    FastBits br = {scan, segs[2 * s], segs[2 * s + 1], 0, 0};
    if (br.end < br.p || (long)(br.end >> 3) + SCAN_PAD > scan_bytes) return E_ARG;
    const int nb = prog_seg_blocks(sc, s);
    long eobrun = 0;
    for (int i = 0; i < nb; ++i) {
      const long j = per * s + i;
      const uint64_t nz = nonzero(j);
      uint64_t corr = 0, fresh = 0, sign = 0;
      int k = sc->ss;
      if (eobrun == 0) {
        while (k <= sc->se) {
          int sym;
          uint32_t v = 0;
          if (!br.symbol(ac, &sym)) return E_STREAM;
          const int r = sym >> 4, sz = sym & 15;
          if (sz) {
            if (sz != 1 || !br.take(1, &v)) return E_STREAM;
          } else if (r != 15) {
            if (!br.take(r, &v)) return E_STREAM;
            eobrun = (1l << r) + v;
            break;
          }
          const uint64_t band = (~0ull << k) & upto_se;      // positions k .. Se
          uint64_t zeros = ~nz & band;
          for (int t = 0; t < r && zeros; ++t) zeros &= zeros - 1;
          const int kk = zeros ? __builtin_ctzll(zeros) : sc->se + 1;       // the (r + 1)-th zero from k on, or past the band
          if (!br.corrections(nz & band & (kk > 63 ? ~0ull : (1ull << kk) - 1), &corr)) return E_STREAM;
          if (sz) {
            if (kk > sc->se) return E_STREAM;
            fresh |= 1ull << kk;
            if (!v) sign |= 1ull << kk;
          }
          k = kk + 1;
        }
      }
      if (eobrun > 0) {
        if (k <= sc->se && !br.corrections(nz & (~0ull << k) & upto_se, &corr)) return E_STREAM;
        --eobrun;
      }
      update(j, corr, fresh, sign);
    }
    if (eobrun || br.end - br.p > 7) return E_STREAM;       // a run past the interval's blocks, or more than the last byte's padding left
  }
  return OK;
}

// the stand-alone form for the device path: masks [nblocks] in the scan's block order (updated), records [nblocks][3]
inline int prog_refine_ac(const pf_jpeg_prog_scan* sc, const uint8_t* scan, long scan_bytes, const uint32_t* segs, uint64_t* masks, uint64_t* records) {
  if (!masks || !records) return E_ARG;
  return prog_refine_ac_core(
      sc, scan, scan_bytes, segs, [&](long j) { return masks[j]; },
      [&](long j, uint64_t corr, uint64_t fresh, uint64_t sign) {
        records[3 * j] = corr;
        records[3 * j + 1] = fresh;
        records[3 * j + 2] = sign;
        masks[j] |= fresh;
      });
}

inline void prog_apply_record(int16_t* blk, uint64_t corr, uint64_t fresh, uint64_t sign, int al) {
  const int p1 = 1 << al;
  for (uint64_t m = corr | fresh; m; m &= m - 1) {
    const int k = __builtin_ctzll(m);
    int16_t* c = blk + ZIGZAG[k];
    if ((fresh >> k) & 1) *c = (int16_t)(((sign >> k) & 1) ? -p1 : p1);
    else *c = (int16_t)(*c + (*c >= 0 ? p1 : -p1));
  }
}

// Sequential decoder of one scan of any kind, applied to coef (int16 [h->nblocks][64], zeroed by the caller before the first scan)
inline int prog_decode_scan(const pf_jpeg_header* h, const pf_jpeg_prog_scan* sc, const uint8_t* scan, long scan_bytes, const uint32_t* segs,
                            int16_t* coef) {
  if (!prog_scan_fits(h, sc) || !scan || !segs || !coef) return E_ARG;
  if (sc->kind == AC_REFINE)
    return prog_refine_ac_core(
        sc, scan, scan_bytes, segs,
        [&](long j) {
          const int16_t* blk = coef + prog_block_index(h, sc, j) * 64;
          uint64_t m = 0;
          for (int k = 0; k < 64; ++k) m |= (uint64_t)(blk[ZIGZAG[k]] != 0) << k;
          return m;
        },
        [&](long j, uint64_t corr, uint64_t fresh, uint64_t sign) { prog_apply_record(coef + prog_block_index(h, sc, j) * 64, corr, fresh, sign, sc->al); });
  HostHuff tab[3];
  int comp[6] = {0, 0, 0, 0, 0, 0};              // index into the scan's components of block b of a unit
  if (sc->kind == DC_FIRST) {
    for (int c = 0; c < sc->ncomp; ++c) tab[c].build(sc->huff_bits[sc->td[c]], sc->huff_vals[sc->td[c]]);
    if (sc->ncomp > 1) block_components(h, comp);
  } else if (sc->kind == AC_FIRST) {
    tab[0].build(sc->huff_bits[4 + sc->ta[0]], sc->huff_vals[4 + sc->ta[0]]);
  }
  const long per = (long)sc->restart_interval * sc->blocks_per_unit;
  const int scale = 1 << sc->al;
  for (int s = 0; s < sc->nsegments; ++s) {
    ProgBits br = {scan, segs[2 * s], segs[2 * s + 1]};
    if (br.end < br.p || (long)(br.end >> 3) + SCAN_PAD > scan_bytes) return E_ARG;
    const int nb = prog_seg_blocks(sc, s);
    int32_t pred[3] = {0, 0, 0};
    long eobrun = 0;
    for (int i = 0; i < nb; ++i) {
      int16_t* blk = coef + prog_block_index(h, sc, per * s + i) * 64;
      int sym, v, b;
      if (sc->kind == DC_FIRST) {
        const int c = comp[i % sc->blocks_per_unit];
        if (!br.symbol(tab[c], &sym) || !br.bits(sym & 15, &v)) return E_STREAM;
        pred[c] += huff_extend(v, sym & 15);
        blk[0] = (int16_t)(pred[c] * scale);
      } else if (sc->kind == DC_REFINE) {
        if (!br.bit(&b)) return E_STREAM;
        if (b) blk[0] = (int16_t)(blk[0] | scale);
      } else {
        if (eobrun > 0) {
          --eobrun;
          continue;
        }
        for (int k = sc->ss; k <= sc->se; ++k) {
          if (!br.symbol(tab[0], &sym)) return E_STREAM;
          const int r = sym >> 4, sz = sym & 15;
          if (sz) {
            k += r;
            if (!br.bits(sz, &v) || k > sc->se) return E_STREAM;        // libjpeg would store past the band: refused
            blk[ZIGZAG[k]] = (int16_t)(huff_extend(v, sz) * scale);
          } else if (r == 15) {
            k += 15;
          } else {
            if (!br.bits(r, &v)) return E_STREAM;
            eobrun = (1l << r) + v - 1;
            break;
          }
        }
      }
    }
    if (eobrun || br.end - br.p > 7) return E_STREAM;
  }
  return OK;
}

// the subsequence plan of a DC-first or AC-first scan: plan() on the scan's own walk
inline int prog_plan(const pf_jpeg_prog_scan* sc, const uint32_t* segs, int S, uint32_t* lanes, long lane_cap, uint32_t* segx, int* nlanes, int* longest) {
  if (!prog_scan_ok(sc)) return E_ARG;
  pf_jpeg_header t;
  memset(&t, 0, sizeof(t));
  t.restart_interval = sc->restart_interval;
  t.blocks_per_mcu = sc->blocks_per_unit;
  t.nblocks = sc->nblocks;
  t.nsegments = sc->nsegments;
  return plan(&t, segs, S, lanes, lane_cap, segx, nlanes, longest);
}

// decode tables of a scan: slot 2 * i = the DC table of its component i (DC-first scans), slot 1 = its AC table (AC-first scans)
inline int prog_build_tables(const pf_jpeg_prog_scan* sc, uint32_t* out) {
  if (!prog_scan_ok(sc) || !out) return E_ARG;
  memset(out, 0, TABLE_WORDS * sizeof(uint32_t));
  memcpy(out + T_ZIGZAG, ZIGZAG, 64);
  if (sc->ss == 0)
    for (int c = 0; c < sc->ncomp; ++c) build_table_slot(sc->huff_bits[sc->td[c]], sc->huff_vals[sc->td[c]], out + 2 * c * T_WORDS);
  else
    build_table_slot(sc->huff_bits[4 + sc->ta[0]], sc->huff_vals[4 + sc->ta[0]], out + T_WORDS);
  return OK;
}

}  // namespace pf_jpeg
