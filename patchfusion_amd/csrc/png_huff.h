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
#pragma once
#include <stdint.h>
#include <string.h>

namespace pf_png {

constexpr int NSYM = 257, EOB = 256, MAX_BITS = 15, TABLE_WORDS = 324, HDR_WORD0 = 260, HDR_BYTES = 256;

// Code lengths of an n-symbol alphabet (n <= 257) limited to max_bits; len[s] = 0 for count 0.  Huffman by two queues over the sorted
// leaves, then the length counts are folded back under the limit (the overflow is moved one level at a time until the Kraft sum is
// 2^max_bits again) and the lengths re-dealt in order of frequency.  A lone used symbol gets a partner of length 1 (the lowest unused
// index), so the code is complete for every input: inflate rejects an incomplete code-length code.
inline void code_lengths(const uint64_t* count, int n, int max_bits, uint8_t* len) {
  int order[NSYM + 1], m = 0;
  uint64_t cnt[NSYM + 1];
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
  uint64_t w[2 * NSYM];
  int parent[2 * NSYM];
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
  int depth[2 * NSYM], num[MAX_BITS + 2] = {0};
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

  // the 258 code lengths (257 literal / length codes + one distance code of length 0) in the run-length alphabet
  uint8_t seq[NSYM + 1], sym[NSYM + 1], extra[NSYM + 1];
  memcpy(seq, len, NSYM);
  seq[NSYM] = 0;
  int ns = 0;
  for (int i = 0; i < NSYM + 1;) {
    int run = 1;
    while (i + run < NSYM + 1 && seq[i + run] == seq[i]) ++run;
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

  BitWriter bw = {reinterpret_cast<uint8_t*>(table + HDR_WORD0), 0};
  bw.put(0, 1);                                                          // BFINAL = 0
  bw.put(2, 2);                                                          // BTYPE = 2, dynamic Huffman
  bw.put(0, 5);                                                          // HLIT: 257 codes
  bw.put(0, 5);                                                          // HDIST: 1 code
  bw.put((uint32_t)(hclen - 4), 4);
  for (int i = 0; i < hclen; ++i) bw.put(cllen[perm[i]], 3);
  for (int i = 0; i < ns; ++i) {
    bw.put(clcode[sym[i]], cllen[sym[i]]);
    if (sym[i] == 16) bw.put(extra[i], 2);
    else if (sym[i] == 17) bw.put(extra[i], 3);
    else if (sym[i] == 18) bw.put(extra[i], 7);
  }
  if (bw.bits > HDR_BYTES * 8) return 1;                                 // cannot happen: <= 1880
  table[NSYM] = (uint32_t)bw.bits;
  return 0;
}

}  // namespace pf_png
