// Stand-alone host program for csrc/png_huff.h (no HIP, no GPU): builds the table for the five histograms of tests/png_ref.py and
// checks lengths, the Kraft sum, the prefix property of the codes and the header size.  tests/test_png_table_cpu.py compiles it with
// -fsanitize=address,undefined and expects a clean exit.
#include <stdio.h>

#include "png_huff.h"

static int check(const char* name, const uint32_t* hist) {
  uint32_t table[pf_png::TABLE_WORDS];
  if (pf_png::build_table(hist, table)) { printf("%s: build_table failed\n", name); return 1; }
  unsigned long kraft = 0;
  int used = 0, maxlen = 0;
  for (int s = 0; s < pf_png::NSYM; ++s) {
    const int len = (int)(table[s] >> 16);
    const int want = hist[s] != 0 || s == pf_png::EOB;
    if (len > pf_png::MAX_BITS || (want && len < 1)) { printf("%s: symbol %d has length %d\n", name, s, len); return 1; }
    if ((table[s] & 0xffffu) >> len) { printf("%s: symbol %d: code wider than its length\n", name, s); return 1; }
    if (len) { kraft += 1ul << (pf_png::MAX_BITS - len); ++used; }
    if (len > maxlen) maxlen = len;
  }
  if (used >= 2 && kraft != (1ul << pf_png::MAX_BITS)) { printf("%s: Kraft sum %lu / 32768\n", name, kraft); return 1; }
  // prefix property on the bit-reversed codes: no code equals the low bits of a longer or equal one
  for (int a = 0; a < pf_png::NSYM; ++a)
    for (int b = 0; b < pf_png::NSYM; ++b) {
      const int la = (int)(table[a] >> 16), lb = (int)(table[b] >> 16);
      if (a == b || !la || !lb || la > lb) continue;
      if (((table[b] & 0xffffu) & ((1u << la) - 1u)) == (table[a] & 0xffffu)) { printf("%s: code %d is a prefix of code %d\n", name, a, b); return 1; }
    }
  const uint32_t bits = table[pf_png::NSYM];
  if (bits < 17 || bits > (uint32_t)pf_png::HDR_BYTES * 8) { printf("%s: header of %u bits\n", name, bits); return 1; }
  const uint8_t* hdr = reinterpret_cast<const uint8_t*>(table + pf_png::HDR_WORD0);
  if ((hdr[0] & 7u) != 4u) { printf("%s: header does not start with BFINAL = 0, BTYPE = 2\n", name); return 1; }
  for (uint32_t i = bits; i < (uint32_t)pf_png::HDR_BYTES * 8; ++i)
    if ((hdr[i >> 3] >> (i & 7)) & 1u) { printf("%s: header bit %u beyond its length is set\n", name, i); return 1; }
  printf("%s: %d codes, longest %d, header %u bits\n", name, used, maxlen, bits);
  return 0;
}

int main() {
  uint32_t h[5][pf_png::NSYM];
  memset(h, 0, sizeof h);
  for (int s = 0; s < pf_png::NSYM; ++s) h[0][s] = 1000;                         // flat
  h[1][65] = 12345; h[1][pf_png::EOB] = 1;                                       // one literal + end-of-block
  h[2][0] = 7; h[2][255] = 900000; h[2][pf_png::EOB] = 3;                        // two literals
  for (int s = 0; s < 28; ++s) h[3][s * 9] = 1u << s;                            // geometric
  h[3][pf_png::EOB] = 5;
  uint32_t a = 1, b = 1;
  for (int s = 0; s < 40; ++s) { h[4][3 + s * 6] = a; const uint32_t c = a + b; a = b; b = c; }   // Fibonacci: 39 deep before limiting
  h[4][pf_png::EOB] = 1;
  static const char* names[5] = {"flat", "one_literal", "two_literals", "geometric", "fibonacci"};
  int bad = 0;
  for (int i = 0; i < 5; ++i) bad += check(names[i], h[i]);
  if (pf_png::build_table(nullptr, nullptr) != 1) { printf("null pointers accepted\n"); ++bad; }
  if (bad) return 1;
  printf("5 histograms ok\n");
  return 0;
}
