// Stand-alone driver of the subsequence decode's host model (csrc/png_host.h over the lane decoder of csrc/png_inflate.h) for the host
// sanitizers (tests/test_png_inflate_par_sanitizer_cpu.py).  Every file named on the command line is parsed; the finder lists the
// candidates; each goes through scan_block and scan_block_par at lanes of 64 and 256 bits (equal records wherever the sequential status
// is S_OK, a non-OK status elsewhere); the chain is walked over the parallel records and inflate_block_par fills lit / ref, which resolve
// to bytes that must carry the Adler-32 the file states.  Then the same on truncated and bit-flipped copies of the deflate data, where
// errors are expected and memory errors are what the sanitizers catch.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "png_host.h"

using namespace pf_pngd;

struct Work {
  HostCodes hc;
  ParWindowHost w;
};

// -> 0 when the stream decoded to `expected` bytes with the stated Adler-32; `mismatch` counts records that differ from the sequential ones
static int inflate_par(const std::vector<uint8_t>& deflate, long expected, uint32_t S, Work& k, int* mismatch) {
  const long n = (long)deflate.size();
  if (n <= 0 || expected <= 0 || expected > (1l << 24)) return PF_PNGD_E_STREAM;
  const std::vector<uint32_t> words = pad_words(deflate.data(), n);
  Bits b(words.data(), (uint32_t)(8 * n));
  std::vector<uint32_t> recs;
  for (uint32_t p = 0; p < b.nbits; ++p) {
    const uint32_t type = (peek(b, p) >> 1) & 3u;
    if (!((p == 0 && type == 1) || (type == 2 && probe_dynamic(b, p)))) continue;
    uint32_t seq[4], par[4];
    scan_block(b, p, 1u << 21, (uint32_t)expected, k.hc.lens, k.hc.lit(), k.hc.dist(), k.hc.offs, seq);
    scan_block_par(b, p, 1u << 21, (uint32_t)expected, S, k.hc, k.w, par);
    const bool fine = (seq[3] & 255u) == S_OK;
    if (fine ? memcmp(seq, par, sizeof(seq)) != 0 : ((par[3] & 255u) == S_OK || par[0] != seq[0])) ++*mismatch;
    recs.insert(recs.end(), par, par + 4);
  }
  std::vector<uint32_t> blocks;                      // start, type, offset, bytes
  uint32_t p = 0;
  long total = 0;
  for (;;) {
    if (p + 3 > b.nbits) return PF_PNGD_E_STREAM;
    const uint32_t head = peek(b, p), type = (head >> 1) & 3u;
    if (type == 3) return PF_PNGD_E_STREAM;
    if (type == 0) {
      const long byte = ((long)p + 3 + 7) / 8;
      if (byte + 4 > n) return PF_PNGD_E_STREAM;
      const uint32_t len = deflate[byte] | (deflate[byte + 1] << 8), nlen = deflate[byte + 2] | (deflate[byte + 3] << 8);
      if ((len ^ nlen) != 0xffffu || byte + 4 + (long)len > n) return PF_PNGD_E_STREAM;
      const uint32_t blk[4] = {(uint32_t)(byte + 4), 0u, (uint32_t)total, len};
      blocks.insert(blocks.end(), blk, blk + 4);
      total += len;
      p = (uint32_t)(8 * (byte + 4 + (long)len));
    } else {
      uint32_t rec[4] = {0, 0, 0, S_INVALID};
      bool found = false;
      for (size_t i = 0; i + 3 < recs.size() && !found; i += 4)
        if (recs[i] == p) { memcpy(rec, &recs[i], sizeof(rec)); found = true; }
      if (!found && type == 1) scan_block_par(b, p, 1u << 21, (uint32_t)expected, S, k.hc, k.w, rec);
      if ((rec[3] & 255u) != S_OK) return (rec[3] & 255u) == S_SIZE ? PF_PNGD_E_SIZE : PF_PNGD_E_STREAM;
      const uint32_t blk[4] = {p, type, (uint32_t)total, rec[2]};
      blocks.insert(blocks.end(), blk, blk + 4);
      total += rec[2];
      p = rec[1];
    }
    if (total > expected) return PF_PNGD_E_SIZE;
    if (head & 1u) break;
  }
  if (total != expected) return PF_PNGD_E_SIZE;
  // exactly `expected` entries: a store past the block's range is a heap overflow the sanitizer reports
  std::vector<uint8_t> lit((size_t)expected, 0);
  std::vector<uint32_t> ref((size_t)expected);
  for (long i = 0; i < expected; ++i) ref[(size_t)i] = (uint32_t)i;
  uint32_t flags = 0, rounds = 0;
  for (size_t i = 0; i < blocks.size(); i += 4) {
    const uint32_t* blk = &blocks[i];
    if (blk[1] == 0) {
      for (uint32_t j = 0; j < blk[3]; ++j) lit[blk[2] + j] = deflate[blk[0] + j];
      continue;
    }
    flags |= inflate_block_par(b, blk, S, k.hc, k.w, lit.data(), ref.data(), &rounds);
  }
  if (flags & PF_PNGD_F_DISTANCE) return PF_PNGD_E_DISTANCE;
  if (flags) return PF_PNGD_E_STREAM;
  for (int r = 0; r < 26; ++r)
    for (long i = 0; i < expected; ++i) {
      if (ref[(size_t)i] > (uint32_t)i) return PF_PNGD_E_STREAM;             // never: a reference points backwards
      ref[(size_t)i] = ref[ref[(size_t)i]];
    }
  std::vector<uint8_t> out((size_t)expected);
  for (long i = 0; i < expected; ++i) out[(size_t)i] = lit[ref[(size_t)i]];
  const long tail = ((long)p + 7) / 8;
  if (tail + 4 > n) return PF_PNGD_E_STREAM;
  return adler32(out.data(), expected) == rd32(deflate.data() + tail) ? 0 : PF_PNGD_E_ADLER;
}

int main(int argc, char** argv) {
  int files = 0, parsed = 0, intact_ok = 0, damaged = 0, damaged_ok = 0, mismatch = 0;
  uint32_t rng = 24680;
  auto next = [&]() { rng = rng * 1664525u + 1013904223u; return rng >> 8; };
  std::unique_ptr<Work> k(new Work);
  const uint32_t lane_bits[2] = {64, 256};
  for (int a = 1; a < argc; ++a) {
    FILE* f = fopen(argv[a], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[a]); return 2; }
    std::vector<uint8_t> d;
    uint8_t buf[4096];
    size_t got;
    while ((got = fread(buf, 1, sizeof buf, f)) > 0) d.insert(d.end(), buf, buf + got);
    fclose(f);
    ++files;
    pf_pngd_header h;
    std::vector<uint8_t> deflate(d.size() + 16);
    long n = 0;
    if (parse(d.data(), (long)d.size(), 1, &h, deflate.data(), (long)d.size(), &n)) continue;      // a refusal of the parser
    ++parsed;
    deflate.resize((size_t)n);
    const long expected = (long)h.inflated_bytes;
    bool ok = true;
    for (uint32_t S : lane_bits) {
      const int rc = inflate_par(deflate, expected, S, *k, &mismatch);
      if (rc) fprintf(stderr, "%s at %u bits: status %d\n", argv[a], S, rc);
      ok = ok && rc == 0;
    }
    intact_ok += ok;
    if (!ok || deflate.size() < 8) continue;
    for (int t = 0; t < 40; ++t) {
      std::vector<uint8_t> c(deflate);
      if (t < 12) c.resize(1 + next() % (deflate.size() - 1));
      else for (int j = 0; j < 1 + (t % 3); ++j) c[next() % c.size()] ^= (uint8_t)(1u << (next() & 7));
      ++damaged;
      damaged_ok += inflate_par(c, expected, lane_bits[t & 1], *k, &mismatch) == 0;
    }
  }
  printf("%d files, %d parsed, %d decoded; %d damaged copies, %d of them still decoded; %d records differ\n", files, parsed, intact_ok, damaged,
         damaged_ok, mismatch);
  return mismatch ? 1 : 0;
}
