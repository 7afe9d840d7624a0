// Stand-alone driver of the progressive half of csrc/jpeg_host.h for the host sanitizers (tests/test_jpeg_prog_sanitizer_cpu.py): every
// file named on the command line goes through the progressive parser, the preparation of every scan, the sequential decoder of all four
// scan kinds, the stand-alone AC-refinement decoder (against the masks of the decode so far, and against arbitrary masks), the subsequence
// plan, the table builder and the block map; then again truncated at every marker boundary and at random lengths, and with single bits of
// scan data flipped.  Errors are expected on the damaged copies; memory errors are what the sanitizers catch.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "jpeg_host.h"

static int run(const std::vector<uint8_t>& d, std::vector<pf_jpeg_prog_scan>* keep) {
  using namespace pf_jpeg;
  pf_jpeg_header h;
  int cap = 1, ns = 0;
  for (size_t i = 0; i + 1 < d.size(); ++i) cap += d[i] == 0xff && d[i + 1] == 0xda;
  std::vector<pf_jpeg_prog_scan> scans((size_t)cap);
  int rc = prog_parse(d.data(), (long)d.size(), &h, scans.data(), cap, &ns);
  if (rc) return rc;
  scans.resize((size_t)ns);
  if (keep) *keep = scans;
  std::vector<int16_t> coef((size_t)h.nblocks * 64, 0);
  int first_error = 0;
  for (const pf_jpeg_prog_scan& sc : scans) {
    const long bytes_cap = (long)sc.end - sc.begin + SCAN_PAD + 4;
    std::vector<uint8_t> bytes((size_t)bytes_cap);
    std::vector<uint32_t> segs(2 * (size_t)sc.nsegments);
    long n = 0;
    rc = prog_prepare_scan(d.data(), (long)d.size(), &sc, bytes.data(), bytes_cap, &n, segs.data());
    if (rc) return rc;
    if (sc.ncomp == 1) {
      std::vector<int32_t> map((size_t)sc.nblocks);
      if (prog_block_map(&h, &sc, map.data())) return -1;
      for (int32_t m : map)
        if (m < 0 || m >= h.nblocks) return -1;
    }
    if (sc.kind == AC_REFINE) {
      std::vector<uint64_t> masks((size_t)sc.nblocks), rec(3 * (size_t)sc.nblocks);
      for (long j = 0; j < sc.nblocks; ++j) {
        const int16_t* blk = coef.data() + prog_block_index(&h, &sc, j) * 64;
        for (int i = 0; i < 64; ++i) masks[(size_t)j] |= (uint64_t)(blk[pf_jpeg::ZIGZAG[i]] != 0) << i;
      }
      const int a = prog_refine_ac(&sc, bytes.data(), n, segs.data(), masks.data(), rec.data());
      for (uint64_t& m : masks) m = 0x5a5a33cc0ff0a5a5ull;               // masks that have nothing to do with the stream
      prog_refine_ac(&sc, bytes.data(), n, segs.data(), masks.data(), rec.data());
      const int b = prog_decode_scan(&h, &sc, bytes.data(), n, segs.data(), coef.data());
      if (a != b) return -2;                                            // the two forms of the decoder agree on what is an error
      rc = b;
    } else {
      rc = prog_decode_scan(&h, &sc, bytes.data(), n, segs.data(), coef.data());
    }
    if (rc && !first_error) first_error = rc;
    if (sc.kind == DC_FIRST || sc.kind == AC_FIRST) {
      int nl = 0, longest = 0;
      for (int S : {32, 1024}) {
        if (prog_plan(&sc, segs.data(), S, nullptr, 0, nullptr, &nl, &longest)) return -1;
        std::vector<uint32_t> lanes(3 * (size_t)nl), segx(4 * (size_t)sc.nsegments);
        if (prog_plan(&sc, segs.data(), S, lanes.data(), nl, segx.data(), &nl, &longest)) return -1;
      }
      std::vector<uint32_t> tables(TABLE_WORDS);
      if (prog_build_tables(&sc, tables.data())) return -1;
    }
  }
  return first_error;
}

int main(int argc, char** argv) {
  int files = 0, intact_ok = 0, damaged = 0, damaged_ok = 0;
  uint32_t rng = 4321;
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
    std::vector<pf_jpeg_prog_scan> scans;
    const int rc = run(d, &scans);
    if (rc < 0) { fprintf(stderr, "%s: internal check %d failed\n", argv[a], rc); return 3; }
    intact_ok += rc == 0;
    std::vector<size_t> cuts;
    for (size_t i = 2; i + 1 < d.size(); ++i)
      if (d[i] == 0xff && d[i + 1] != 0 && d[i + 1] != 0xff) { cuts.push_back(i); cuts.push_back(i + 1); cuts.push_back(i + 2); cuts.push_back(i + 4); }
    for (int t = 0; t < 40 && d.size() > 2; ++t) cuts.push_back(2 + next() % (d.size() - 2));
    for (size_t cut : cuts) {
      if (cut >= d.size()) continue;
      std::vector<uint8_t> c(d.begin(), d.begin() + (long)cut);
      ++damaged;
      const int r = run(c, nullptr);
      if (r < 0) { fprintf(stderr, "%s cut at %zu: internal check %d failed\n", argv[a], cut, r); return 3; }
      damaged_ok += r == 0;
    }
    for (int t = 0; t < 300 && !scans.empty(); ++t) {
      std::vector<uint8_t> c(d);
      const pf_jpeg_prog_scan& sc = scans[next() % scans.size()];
      if (sc.end <= sc.begin) continue;
      c[(size_t)sc.begin + next() % (size_t)(sc.end - sc.begin)] ^= (uint8_t)(1u << (next() & 7));
      ++damaged;
      const int r = run(c, nullptr);
      if (r < 0) { fprintf(stderr, "%s bit flip: internal check %d failed\n", argv[a], r); return 3; }
      damaged_ok += r == 0;
    }
  }
  printf("%d files, %d decoded; %d damaged copies, %d of them still decoded\n", files, intact_ok, damaged, damaged_ok);
  return 0;
}
