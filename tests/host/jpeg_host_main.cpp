// Stand-alone driver of csrc/jpeg_host.h for the host sanitizers (tests/test_jpeg_sanitizer_cpu.py): every file named on the command line
// goes through the parser, scan preparation, the sequential entropy decoder, the subsequence plan and the table builder, then again
// truncated at many lengths and with bits flipped.  Errors are expected on the damaged copies; memory errors are what the sanitizers catch.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "jpeg_host.h"

static int run(const std::vector<uint8_t>& d) {
  pf_jpeg_header h;
  int rc = pf_jpeg::parse(d.data(), (long)d.size(), &h);
  if (rc) return rc;
  const long cap = (long)d.size() - h.scan_begin + pf_jpeg::SCAN_PAD + 4;
  std::vector<uint8_t> scan((size_t)cap);
  std::vector<uint32_t> segs(2 * (size_t)h.nsegments);
  long n = 0;
  rc = pf_jpeg::prepare_scan(d.data(), (long)d.size(), &h, scan.data(), cap, &n, segs.data());
  if (rc) return rc;
  std::vector<int16_t> coef((size_t)h.nblocks * 64);
  rc = pf_jpeg::decode_entropy(&h, scan.data(), n, segs.data(), coef.data());
  int nl = 0, longest = 0;
  for (int S : {32, 1024}) {
    if (pf_jpeg::plan(&h, segs.data(), S, nullptr, 0, nullptr, &nl, &longest)) return -1;
    std::vector<uint32_t> lanes(3 * (size_t)nl), segx(4 * (size_t)h.nsegments);
    if (pf_jpeg::plan(&h, segs.data(), S, lanes.data(), nl, segx.data(), &nl, &longest)) return -1;
  }
  std::vector<uint32_t> tables(pf_jpeg::TABLE_WORDS);
  if (pf_jpeg::build_tables(&h, tables.data())) return -1;
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
    const int rc = run(d);
    if (rc < 0) { fprintf(stderr, "%s: plan or tables failed\n", argv[a]); return 3; }
    intact_ok += rc == 0;
    for (int t = 0; t < 60 && d.size() > 2; ++t) {
      std::vector<uint8_t> c(d.begin(), d.begin() + 2 + next() % (d.size() - 2));
      ++damaged;
      damaged_ok += run(c) == 0;
    }
    for (int t = 0; t < 200; ++t) {
      std::vector<uint8_t> c(d);
      for (int k = 0; k < 3; ++k) c[next() % c.size()] ^= (uint8_t)(1u << (next() & 7));
      ++damaged;
      damaged_ok += run(c) == 0;
    }
  }
  printf("%d files, %d decoded; %d damaged copies, %d of them still decoded\n", files, intact_ok, damaged, damaged_ok);
  return 0;
}
