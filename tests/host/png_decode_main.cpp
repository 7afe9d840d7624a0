// Stand-alone driver of csrc/png_host.h and csrc/png_inflate.h for the host sanitizers (tests/test_png_decode_sanitizer_cpu.py): every file
// named on the command line goes through the chunk parser and the sequential restatement of the device inflate (finder at every bit, scan
// records, chain walk, references, pointer jumping), whose output must carry the Adler-32 the file states; then again truncated at many
// lengths and with bits flipped, in the file and in the deflate data itself (which no CRC guards here).  Errors are expected on the
// damaged copies; memory errors are what the sanitizers catch.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "png_host.h"

static int inflate_checked(const std::vector<uint8_t>& deflate, long expected) {
  std::vector<uint8_t> out((size_t)expected);
  long stats[6];
  const int rc = pf_pngd::inflate_model(deflate.data(), (long)deflate.size(), expected, 1u << 21, out.data(), stats);
  if (rc) return rc;
  if (stats[5] + 4 > (long)deflate.size()) return PF_PNGD_E_STREAM;
  return pf_pngd::adler32(out.data(), expected) == pf_pngd::rd32(deflate.data() + stats[5]) ? 0 : PF_PNGD_E_ADLER;
}

static int run(const std::vector<uint8_t>& d, std::vector<uint8_t>* deflate_out, long* expected_out) {
  pf_pngd_header h;
  std::vector<uint8_t> deflate(d.size() + 16);
  long n = 0;
  int rc = pf_pngd::parse(d.data(), (long)d.size(), 1, &h, deflate.data(), (long)d.size(), &n);
  if (rc) return rc;
  if (h.inflated_bytes > (1l << 24)) return -1;          // the fixture files are small
  deflate.resize((size_t)n);
  rc = inflate_checked(deflate, (long)h.inflated_bytes);
  if (deflate_out) { *deflate_out = deflate; *expected_out = (long)h.inflated_bytes; }
  return rc;
}

int main(int argc, char** argv) {
  int files = 0, intact_ok = 0, damaged = 0, damaged_ok = 0;
  uint32_t rng = 12345;
  auto next = [&]() { rng = rng * 1664525u + 1013904223u; return rng >> 8; };
  for (int a = 1; a < argc; ++a) {
    FILE* f = fopen(argv[a], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[a]); return 2; }
    std::vector<uint8_t> d;
    uint8_t buf[4096];
    size_t got;
    while ((got = fread(buf, 1, sizeof buf, f)) > 0) d.insert(d.end(), buf, buf + got);
    fclose(f);
    ++files;
    std::vector<uint8_t> deflate;
    long expected = 0;
    const int rc = run(d, &deflate, &expected);
    if (rc < 0) { fprintf(stderr, "%s: too large for this driver\n", argv[a]); return 3; }
    if (rc) fprintf(stderr, "%s: status %d\n", argv[a], rc);
    intact_ok += rc == 0;
    for (int t = 0; t < 20 && d.size() > 8; ++t) {
      std::vector<uint8_t> c(d.begin(), d.begin() + 8 + next() % (d.size() - 8));
      ++damaged;
      damaged_ok += run(c, nullptr, nullptr) == 0;
    }
    for (int t = 0; t < 20; ++t) {
      std::vector<uint8_t> c(d);
      for (int k = 0; k < 3; ++k) c[next() % c.size()] ^= (uint8_t)(1u << (next() & 7));
      ++damaged;
      damaged_ok += run(c, nullptr, nullptr) == 0;
    }
    if (rc || deflate.size() < 8) continue;
    for (int t = 0; t < 20; ++t) {
      std::vector<uint8_t> c(deflate.begin(), deflate.begin() + 1 + next() % (deflate.size() - 1));
      ++damaged;
      damaged_ok += inflate_checked(c, expected) == 0;
    }
    for (int t = 0; t < 60; ++t) {
      std::vector<uint8_t> c(deflate);
      const int flips = 1 + (t % 3);
      for (int k = 0; k < flips; ++k) c[next() % c.size()] ^= (uint8_t)(1u << (next() & 7));
      ++damaged;
      damaged_ok += inflate_checked(c, expected) == 0;
    }
  }
  printf("%d files, %d decoded; %d damaged copies, %d of them still decoded\n", files, intact_ok, damaged, damaged_ok);
  return 0;
}
