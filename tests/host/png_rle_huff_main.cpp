// Stand-alone host program for the run-match table builder of csrc/png_huff.h (no HIP, no GPU): builds the 286-symbol table for the
// histograms of tests/png_ref.py extended with length-symbol counts and checks lengths against the 14-bit limit, the Kraft sum, the
// prefix property, the length-symbol words, the distance code, HLIT and the header size.  It also rebuilds the literal table beside
// it, so that both builders run under the sanitizers in one process.  tests/test_png_rle_cpu.py compiles it with
// -fsanitize=address,undefined and expects a clean exit.
#include <stdio.h>

#include "png_huff.h"

static const int kBase[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
static const int kExtra[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};

static int check(const char* name, const uint32_t* hist) {
  uint32_t table[pf_png::RLE_TABLE_WORDS];
  if (pf_png::build_rle_table(hist, table)) { printf("%s: build_rle_table failed\n", name); return 1; }
  unsigned long kraft = 0;
  int used = 0, maxlen = 0, top = pf_png::NSYM;
  for (int s = 0; s < pf_png::RLE_NSYM; ++s) {
    const int len = (int)(table[s] >> 16);
    const int want = hist[s] != 0 || s == pf_png::EOB;
    if (len > pf_png::RLE_MAX_BITS || (want && len < 1)) { printf("%s: symbol %d has length %d\n", name, s, len); return 1; }
    if ((table[s] & 0xffffu) >> len) { printf("%s: symbol %d: code wider than its length\n", name, s); return 1; }
    if (len) { kraft += 1ul << (pf_png::RLE_MAX_BITS - len); ++used; }
    if (len > maxlen) maxlen = len;
    if (len && s >= pf_png::NSYM) top = s + 1;
  }
  if (used >= 2 && kraft != (1ul << pf_png::RLE_MAX_BITS)) { printf("%s: Kraft sum %lu / 16384\n", name, kraft); return 1; }
  for (int a = 0; a < pf_png::RLE_NSYM; ++a)
    for (int b = 0; b < pf_png::RLE_NSYM; ++b) {
      const int la = (int)(table[a] >> 16), lb = (int)(table[b] >> 16);
      if (a == b || !la || !lb || la > lb) continue;
      if (((table[b] & 0xffffu) & ((1u << la) - 1u)) == (table[a] & 0xffffu)) { printf("%s: code %d is a prefix of code %d\n", name, a, b); return 1; }
    }
  for (int k = 0; k < 29; ++k)
    if (table[pf_png::RLE_LEN_WORD0 + k] != ((uint32_t)kBase[k] | ((uint32_t)kExtra[k] << 16))) { printf("%s: length symbol %d\n", name, 257 + k); return 1; }
  if (table[pf_png::RLE_DIST_WORD] != (1u << 16)) { printf("%s: distance code\n", name); return 1; }
  const uint32_t bits = table[pf_png::RLE_HDR_BITS_WORD];
  if (bits < 17 || bits > 3 + 14 + 57 + 287 * 7) { printf("%s: header of %u bits\n", name, bits); return 1; }
  const uint8_t* hdr = reinterpret_cast<const uint8_t*>(table + pf_png::RLE_HDR_WORD0);
  if ((hdr[0] & 7u) != 4u) { printf("%s: header does not start with BFINAL = 0, BTYPE = 2\n", name); return 1; }
  if ((int)(hdr[0] >> 3) != top - pf_png::NSYM) { printf("%s: HLIT %d, want %d\n", name, hdr[0] >> 3, top - pf_png::NSYM); return 1; }
  for (uint32_t i = bits; i < (uint32_t)pf_png::RLE_HDR_BYTES * 8; ++i)
    if ((hdr[i >> 3] >> (i & 7)) & 1u) { printf("%s: header bit %u beyond its length is set\n", name, i); return 1; }
  uint32_t literal[pf_png::TABLE_WORDS];
  if (pf_png::build_table(hist, literal)) { printf("%s: build_table failed\n", name); return 1; }
  printf("%s: %d codes, longest %d, HLIT %d, header %u bits\n", name, used, maxlen, top - pf_png::NSYM, bits);
  return 0;
}

int main() {
  static uint32_t h[7][pf_png::RLE_NSYM];
  memset(h, 0, sizeof h);
  for (int s = 0; s < pf_png::RLE_NSYM; ++s) h[0][s] = 1000;                     // flat: every symbol, HLIT = 29
  h[1][65] = 12345; h[1][pf_png::EOB] = 1;                                       // one literal + end-of-block, no matches
  h[2][0] = 7; h[2][255] = 900000; h[2][pf_png::EOB] = 3; h[2][285] = 40000;     // two literals and the longest match
  for (int s = 0; s < 28; ++s) h[3][s * 9] = 1u << s;                            // geometric, lengths up to symbol 269
  h[3][pf_png::EOB] = 5;
  for (int k = 0; k < 13; ++k) h[3][257 + k] = 3 + k;
  uint32_t a = 1, b = 1;
  for (int s = 0; s < 40; ++s) { h[4][3 + s * 6] = a; const uint32_t c = a + b; a = b; b = c; }   // Fibonacci: 39 deep before limiting
  h[4][pf_png::EOB] = 1;
  for (int k = 0; k < 29; ++k) h[4][257 + k] = 1 + k;
  h[5][pf_png::EOB] = 1; h[5][0] = 1; h[5][285] = 4000000000u;                   // an all-zero image: matches dominate
  h[6][0] = 1;                                                                   // the end-of-block count missing
  static const char* names[7] = {"flat", "one_literal", "two_literals", "geometric", "fibonacci", "zeros", "no_eob"};
  int bad = 0;
  for (int i = 0; i < 7; ++i) bad += check(names[i], h[i]);
  if (pf_png::build_rle_table(nullptr, nullptr) != 1) { printf("null pointers accepted\n"); ++bad; }
  if (bad) return 1;
  printf("7 histograms ok\n");
  return 0;
}
