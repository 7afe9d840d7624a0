// Host side of the device PNG encoder (csrc/png.hip): from the 257-bin histogram of the filtered stream (256 literals + end-of-block)
// to a canonical Huffman code limited to 15 bits and the bit string of the dynamic-block header that announces it (RFC 1951 3.2.7).
// Plain C++, no HIP, no allocation: compiled into libpf_hip.so through png.hip and, stand-alone, by tests/host/png_huff_main.cpp.
//
// Table layout (PF_PNG_TABLE_WORDS = 324 uint32):
//   [0 .. 256]   symbol s: (code, bit-reversed so that its first bit is bit 0) | length << 16      (length 0 = unused symbol)
//   [257]        number of bits of the block header
//   [258 .. 259] zero
//   [260 .. 323] the block header, 256 bytes, first bit = bit 0 of byte 0, zero-padded: BFINAL = 0, BTYPE = 2, HLIT = 0 (257 codes),
//                HDIST = 0 (one distance code, of length zero: the block has no matches), HCLEN, the code-length code, the 258 lengths
//                with the run symbols 16 / 17 / 18.  At most 3 + 14 + 57 + 258 * 7 = 1880 bits.
//
// Second builder, for the run-match coding of csrc/png_rle.hip (matches at distance 1 only): the 286-symbol literal / length alphabet
// limited to RLE_MAX_BITS = 14, so that the three literals and one match that four consecutive stream positions can emit stay inside
// the 64-bit word a lane merges (3 * 14 + 14 + 5 + 1 = 62 bits).  Table layout (PF_PNG_RLE_TABLE_WORDS = 388 uint32):
//   [0 .. 285]   symbol s: bit-reversed code | length << 16 (0 = unused); 256 = end-of-block, 257 .. 285 the length symbols
//   [286]        number of bits of the block header
//   [287]        the distance code of symbol 0 (distance 1): code 0 | 1 << 16
//   [288 .. 316] length symbol 257 + k: base length | extra bits << 16 (RFC 1951 3.2.5)
//   [317 .. 319] zero
//   [320 .. 387] the block header, 272 bytes: HLIT = highest used length symbol - 256 (0 .. 29), HDIST = 0 with ONE distance code of
//                length 1 (a lone distance code may be incomplete), HCLEN, the code-length code, 257 + HLIT + 1 lengths.  At most
//                3 + 14 + 57 + 287 * 7 = 2083 bits.
#pragma once
#include <stdint.h>
#include <string.h>

namespace pf_png {

constexpr int NSYM = 257, EOB = 256, MAX_BITS = 15, TABLE_WORDS = 324, HDR_WORD0 = 260, HDR_BYTES = 256;
constexpr int RLE_NSYM = 286, RLE_MAX_BITS = 14, RLE_TABLE_WORDS = 388, RLE_HDR_BITS_WORD = 286, RLE_DIST_WORD = 287, RLE_LEN_WORD0 = 288,
              RLE_HDR_WORD0 = 320, RLE_HDR_BYTES = 272;
constexpr int MAX_NSYM = RLE_NSYM;                                         // the larger alphabet sizes the work arrays below

// Code lengths of an n-symbol alphabet (n <= MAX_NSYM) limited to max_bits; len[s] = 0 for count 0.  Huffman by two queues over the sorted
// leaves, then the length counts are folded back under the limit (the overflow is moved one level at a time until the Kraft sum is
// 2^max_bits again) and the lengths re-dealt in order of frequency.  A lone used symbol gets a partner of length 1 (the lowest unused
// index), so the code is complete for every input: inflate rejects an incomplete code-length code.
inline void code_lengths(const uint64_t* count, int n, int max_bits, uint8_t* len) {
  int order[MAX_NSYM + 1], m = 0;
  uint64_t cnt[MAX_NSYM + 1];
  for (int s = 0; s < n; ++s) { len[s] = 0; cnt[s] = count[s]; }
  for (int s = 0; s < n; ++s) if (cnt[s]) ++m;
  for (int s = 0; m < 2 && s < n; ++s) if (!cnt[s]) { cnt[s] = 1; ++m; }     // n >= 2 always
  m = 0;
  for (int s = 0; s < n; ++s) if (cnt[s]) order[m++] = s;
  for (int i = 1; i < m; ++i) {                                          // insertion sort, ascending count, ties by index
    const int s = order[i];
    int j = i;
    for (; j > 0 && cnt[order[j - 1]] > cnt[s]; --j) order[j] = order[j - 1];
    order[j] = s;
  }
  // nodes 0 .. m-1 are the sorted leaves, m .. 2m-2 the internal nodes in order of creation (non-decreasing weight)
  uint64_t w[2 * MAX_NSYM];
  int parent[2 * MAX_NSYM];
  for (int i = 0; i < m; ++i) w[i] = cnt[order[i]];
  int leaf = 0, inner = m, next = m;
  for (; next < 2 * m - 1; ++next) {
    int pick[2];
    for (int k = 0; k < 2; ++k) {
      if (leaf < m && (inner >= next || w[leaf] <= w[inner])) pick[k] = leaf++;
      else pick[k] = inner++;
    }
    w[next] = w[pick[0]] + w[pick[1]];
    parent[pick[0]] = parent[pick[1]] = next;
  }
  int depth[2 * MAX_NSYM], num[MAX_BITS + 2] = {0};
  depth[2 * m - 2] = 0;
  for (int i = 2 * m - 3; i >= 0; --i) depth[i] = depth[parent[i]] + 1;      // a parent always has the larger index
  for (int i = 0; i < m; ++i) num[depth[i] > max_bits ? max_bits : depth[i]]++;
  // depths above the limit were counted at the limit: the Kraft sum (in units of 2^-max_bits) is now too large by `total - 2^max_bits`
  uint64_t total = 0;
  for (int l = 1; l <= max_bits; ++l) total += (uint64_t)num[l] << (max_bits - l);
  while (total > ((uint64_t)1 << max_bits)) {
    num[max_bits]--;                                                     // one code of the longest length leaves ...
    for (int l = max_bits - 1; l >= 1; --l)
      if (num[l]) { num[l]--; num[l + 1] += 2; break; }                  // ... and pairs up with a shorter one, one level down
    total--;
  }
  // least frequent symbols take the longest codes
  int i = 0;
  for (int l = max_bits; l >= 1; --l)
    for (int k = 0; k < num[l]; ++k) len[order[i++]] = (uint8_t)l;
}

// canonical codes (RFC 1951 3.2.2), returned bit-reversed: deflate packs Huffman codes starting from their most significant bit
inline void canonical_codes(const uint8_t* len, int n, int max_bits, uint16_t* code) {
  int bl_count[MAX_BITS + 2] = {0};
  uint32_t next_code[MAX_BITS + 2] = {0};
  for (int s = 0; s < n; ++s) bl_count[len[s]]++;
  bl_count[0] = 0;
  uint32_t c = 0;
  for (int b = 1; b <= max_bits; ++b) { c = (c + bl_count[b - 1]) << 1; next_code[b] = c; }
  for (int s = 0; s < n; ++s) {
    code[s] = 0;
    if (!len[s]) continue;
    uint32_t v = next_code[len[s]]++, r = 0;
    for (int b = 0; b < len[s]; ++b) r |= ((v >> b) & 1u) << (len[s] - 1 - b);
    code[s] = (uint16_t)r;
  }
}

struct BitWriter {
  uint8_t* p;
  int bits;
  void put(uint32_t v, int n) {                                          // n <= 16 bits, least significant first
    for (int b = 0; b < n; ++b, ++bits)
      if ((v >> b) & 1u) p[bits >> 3] |= (uint8_t)(1u << (bits & 7));
  }
};

// The dynamic-block header for the n code lengths of seq (the literal / length codes followed by the distance codes, n <= MAX_NSYM + 1),
// announced as HLIT = hlit and HDIST = 0: the lengths in the run-length alphabet 0 .. 15, 16 / 17 / 18, coded with a code of <= 7 bits.
inline void put_block_header(BitWriter& bw, const uint8_t* seq, int n, int hlit) {
  uint8_t sym[MAX_NSYM + 1], extra[MAX_NSYM + 1];
  int ns = 0;
  for (int i = 0; i < n;) {
    int run = 1;
    while (i + run < n && seq[i + run] == seq[i]) ++run;
    const int v = seq[i];
    i += run;
    if (v == 0) {
      while (run >= 11) { const int r = run > 138 ? 138 : run; sym[ns] = 18; extra[ns++] = (uint8_t)(r - 11); run -= r; }
      if (run >= 3) { sym[ns] = 17; extra[ns++] = (uint8_t)(run - 3); run = 0; }
      while (run-- > 0) { sym[ns] = 0; extra[ns++] = 0; }
    } else {
      sym[ns] = (uint8_t)v; extra[ns++] = 0; --run;                      // the value itself, then repeats of it
      while (run >= 3) { const int r = run > 6 ? 6 : run; sym[ns] = 16; extra[ns++] = (uint8_t)(r - 3); run -= r; }
      while (run-- > 0) { sym[ns] = (uint8_t)v; extra[ns++] = 0; }
    }
  }
  uint64_t clcount[19] = {0};
  for (int i = 0; i < ns; ++i) clcount[sym[i]]++;
  uint8_t cllen[19];
  uint16_t clcode[19];
  code_lengths(clcount, 19, 7, cllen);
  canonical_codes(cllen, 19, 7, clcode);
  static const uint8_t perm[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
  int hclen = 19;
  while (hclen > 4 && !cllen[perm[hclen - 1]]) --hclen;

  bw.put(0, 1);                                                          // BFINAL = 0
  bw.put(2, 2);                                                          // BTYPE = 2, dynamic Huffman
  bw.put((uint32_t)hlit, 5);                                             // HLIT: 257 + hlit literal / length codes
  bw.put(0, 5);                                                          // HDIST: 1 code
  bw.put((uint32_t)(hclen - 4), 4);
  for (int i = 0; i < hclen; ++i) bw.put(cllen[perm[i]], 3);
  for (int i = 0; i < ns; ++i) {
    bw.put(clcode[sym[i]], cllen[sym[i]]);
    if (sym[i] == 16) bw.put(extra[i], 2);
    else if (sym[i] == 17) bw.put(extra[i], 3);
    else if (sym[i] == 18) bw.put(extra[i], 7);
  }
}

// hist: 257 counts (symbol 256 = end-of-block; a zero there is counted as one, every block ends with it).  table: TABLE_WORDS words out.
inline int build_table(const uint32_t* hist, uint32_t* table) {
  if (!hist || !table) return 1;
  uint64_t count[NSYM];
  for (int s = 0; s < NSYM; ++s) count[s] = hist[s];
  if (!count[EOB]) count[EOB] = 1;
  uint8_t len[NSYM];
  uint16_t code[NSYM];
  code_lengths(count, NSYM, MAX_BITS, len);
  canonical_codes(len, NSYM, MAX_BITS, code);
  memset(table, 0, TABLE_WORDS * sizeof(uint32_t));
  for (int s = 0; s < NSYM; ++s) table[s] = (uint32_t)code[s] | ((uint32_t)len[s] << 16);

  // the 258 code lengths: 257 literal / length codes + one distance code of length 0 (the block has no matches)
  uint8_t seq[NSYM + 1];
  memcpy(seq, len, NSYM);
  seq[NSYM] = 0;
  BitWriter bw = {reinterpret_cast<uint8_t*>(table + HDR_WORD0), 0};
  put_block_header(bw, seq, NSYM + 1, 0);
  if (bw.bits > HDR_BYTES * 8) return 1;                                 // cannot happen: <= 1880
  table[NSYM] = (uint32_t)bw.bits;
  return 0;
}

// length symbol 257 + k of RFC 1951 3.2.5: base length and number of extra bits
inline int length_base(int k) { return k < 8 ? 3 + k : (k == 28 ? 258 : 3 + ((4 + (k & 3)) << (k / 4 - 1))); }
inline int length_extra_bits(int k) { return (k < 8 || k == 28) ? 0 : k / 4 - 1; }

// hist: RLE_NSYM token counts (literals, [256] = end-of-block, counted as one if zero, [257 ..] = matches by length symbol).
// table: RLE_TABLE_WORDS words out (layout above).
inline int build_rle_table(const uint32_t* hist, uint32_t* table) {
  if (!hist || !table) return 1;
  uint64_t count[RLE_NSYM];
  for (int s = 0; s < RLE_NSYM; ++s) count[s] = hist[s];
  if (!count[EOB]) count[EOB] = 1;
  uint8_t len[RLE_NSYM];
  uint16_t code[RLE_NSYM];
  code_lengths(count, RLE_NSYM, RLE_MAX_BITS, len);
  canonical_codes(len, RLE_NSYM, RLE_MAX_BITS, code);
  memset(table, 0, RLE_TABLE_WORDS * sizeof(uint32_t));
  for (int s = 0; s < RLE_NSYM; ++s) table[s] = (uint32_t)code[s] | ((uint32_t)len[s] << 16);
  table[RLE_DIST_WORD] = 1u << 16;
  for (int k = 0; k < 29; ++k) table[RLE_LEN_WORD0 + k] = (uint32_t)length_base(k) | ((uint32_t)length_extra_bits(k) << 16);

  int nlit = RLE_NSYM;                                                   // trailing unused length symbols are not announced
  while (nlit > NSYM && !len[nlit - 1]) --nlit;
  uint8_t seq[RLE_NSYM + 1];
  memcpy(seq, len, nlit);
  seq[nlit] = 1;                                                         // the one distance code
  BitWriter bw = {reinterpret_cast<uint8_t*>(table + RLE_HDR_WORD0), 0};
  put_block_header(bw, seq, nlit + 1, nlit - NSYM);
  if (bw.bits > RLE_HDR_BYTES * 8) return 1;                             // cannot happen: <= 2083
  table[RLE_HDR_BITS_WORD] = (uint32_t)bw.bits;
  return 0;
}

}  // namespace pf_png
