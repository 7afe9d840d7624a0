// Progressive JPEG on the device (include/pf_hip.h, "progressive JPEG"): the scan kinds whose decoder state does not depend on earlier scans
// run here, scan after scan on one stream, into the coefficient array csrc/jpeg.hip reconstructs from.  Parsing, scan preparation, the
// plans, the tables, the block maps and the AC-refinement decoder are host code (jpeg_host.h).
//
// DC-first and AC-first scans are Huffman streams decoded in self-synchronising subsequences exactly as jpeg.hip decodes a baseline scan
// (rounds over double-buffered exit states until none changes, a lane scan, a write pass).  A lane's state is (p, s): bit position and,
// for a DC-first scan, the block inside the MCU (always 0 in a one-component scan); for an AC-first scan the zigzag position, Ss = a block
// starts.  An end-of-band run completes the block it stands in and run - 1 more that consume no bits: the whole run is added to the lane's
// block count at once and the state goes to the start of a block, so a pending run is never part of a state and two lanes that agree from
// some bit on hold equal states.  Block counts live in their own words and saturate at 2^30, above any scan's block count.
// A DC-first write pass stores the differences in the scan's own block order; a segmented scan (jpeg_dev.h) then makes them absolute per
// component and stores them shifted by Al through the block map.  DC refinement is closed-form: inside a restart interval bit i belongs
// to block i.  AC refinement is decoded on the host against non-zero masks made here, and its records are applied here.
//
// Termination and bounds (the invariants every kernel below keeps):
//   * every decoder step consumes at least one bit or leaves the loop: a code that matches no table entry consumes one bit and sets nothing;
//   * a symbol (with its extra bits) that would run past its segment's end ends the lane in front of it;
//   * every decode loop runs while p < end, so it is bounded by S plus one symbol;
//   * the zigzag position indexes the zigzag table only after it was found <= Se <= 63; a run past the band stores nothing and is an error;
//   * an end-of-band run is added to a saturating block count; a coefficient or difference is stored only for a block index below its
//     segment's first block + block count, which lies inside the scan's walk, and the block map sends that into the coefficient array;
//   * every 64-bit window read lies inside the scan buffer: p < segment end <= 8 * (scan_bytes - SCAN_PAD); the DC-refinement kernel
//     checks its bit position against both the segment's end and the buffer;
//   * the host's round loop is bounded per scan by that scan's longest segment in lanes and by max_sync_rounds;
//   * no kernel waits for another: every dependency is a kernel boundary on the one stream.
#include "pf_common.h"
#include "../../include/pf_hip.h"
#include "jpeg_host.h"
#include "jpeg_dev.h"

namespace {

using namespace pf_jpeg;

constexpr uint32_t COUNT_CAP = 1u << 30;     // block counts saturate here: two of them still add up inside 32 bits

struct ScanGeom {
  int ss, se, al, bpu, nblocks, segblocks;   // segblocks = restart interval * bpu, or nblocks without restart intervals
  uint32_t comp_of;                          // 2 bits per block of a unit: index into the scan's components
};

__device__ __forceinline__ uint32_t sat_add(uint32_t a, uint32_t b) { return min(a + b, COUNT_CAP); }
__device__ __forceinline__ long block_at(const int32_t* __restrict__ map, uint32_t j) { return map ? (long)map[j] : (long)j; }

// Decodes from (p, st) while p < end.  WRITE: blocks [blk, limit) receive their values (DC differences -> diff in scan order, AC
// coefficients shifted by Al -> coef through the map); the lane stops at blk >= limit; an invalid code (1), more than 7 bits left over
// at the limit (2), a run past the limit (4) or past the band (8) raise *err.
template <bool AC, bool WRITE>
__device__ __forceinline__ void prog_lane(const uint32_t* __restrict__ scan, const uint32_t* tab, const ScanGeom& g, uint32_t& p, int& st, uint32_t& n,
                                          uint32_t end, uint32_t seg_end, int* __restrict__ diff, int16_t* __restrict__ coef,
                                          const int32_t* __restrict__ map, uint32_t& blk, uint32_t limit, uint32_t* err) {
  const uint8_t* zz = reinterpret_cast<const uint8_t*>(tab + T_ZIGZAG);
  uint32_t wi = 0xffffffffu, hi = 0, lo = 0;
  while (p < end) {
    if (WRITE && blk >= limit) break;
    if ((p >> 5) != wi) {
      wi = p >> 5;
      hi = __builtin_bswap32(scan[wi]);
      lo = __builtin_bswap32(scan[wi + 1]);
    }
    const uint32_t win = (p & 31u) ? (hi << (p & 31u)) | (lo >> (32u - (p & 31u))) : hi;
    const uint32_t* T = tab + (AC ? 1u : 2u * ((g.comp_of >> (2 * st)) & 3u)) * T_WORDS;
    const uint32_t e = reinterpret_cast<const uint16_t*>(T + T_LOOK)[win >> (32 - LOOK_BITS)];
    uint32_t len = e >> 8, sym = e & 255u;
    if (!e) {
      const int32_t* maxcode = reinterpret_cast<const int32_t*>(T + T_MAXCODE);
      for (int l = LOOK_BITS + 1; l <= 16; ++l) {
        const int32_t code = (int32_t)(win >> (32 - l));
        if (code <= maxcode[l]) {
          len = l;
          sym = reinterpret_cast<const uint8_t*>(T + T_VALS)[(code + reinterpret_cast<const int32_t*>(T + T_VALOFF)[l]) & 255];
          break;
        }
      }
    }
    if (len == 0) {                       // no such code: one bit consumed, nothing set
      if (WRITE) atomicOr(err, 1u);
      ++p;
      continue;
    }
    const uint32_t r = sym >> 4, sz = sym & 15u;
    const uint32_t extra = (!AC || sz) ? sz : (r < 15u ? r : 0u);
    if (p + len + extra > seg_end) break;
    const uint32_t bits = extra ? ((win << len) >> (32u - extra)) : 0u;        // len + extra <= 31
    p += len + extra;
    const int val = sz ? (bits < (1u << (sz - 1)) ? (int)bits - (1 << sz) + 1 : (int)bits) : 0;
    uint32_t done;
    if (!AC) {
      if (WRITE) diff[blk] = val;
      st = (st + 1 == g.bpu) ? 0 : st + 1;
      done = 1;
    } else if (sz) {
      st += (int)r;
      if (st <= g.se) {
        if (WRITE) coef[block_at(map, blk) * 64 + zz[st]] = (int16_t)(val * (1 << g.al));
      } else if (WRITE) {
        atomicOr(err, 8u);
      }
      ++st;
      done = st > g.se;
    } else if (r == 15u) {
      st += 16;
      done = st > g.se;
    } else {
      done = (1u << r) + bits;            // the block the run stands in and run - 1 more: no bits of theirs follow
    }
    if (done) {
      if (AC) st = g.ss;
      n = sat_add(n, done);
      blk = sat_add(blk, done);
      if (WRITE && blk > limit) atomicOr(err, 4u);
      if (WRITE && blk >= limit && seg_end - p > 7u) atomicOr(err, 2u);
    }
  }
}

// round 0 (first != 0): every lane from (its start, a block starts).  Later rounds: every lane that is not the first of its segment from
// the exit state the lane before it had after the round before; flags[0] counts the exits (state or block count) that changed.
template <bool AC>
__global__ __launch_bounds__(JT) void jpeg_prog_sync_kernel(const uint32_t* __restrict__ scan, const uint32_t* __restrict__ tables,
                                                             const uint32_t* __restrict__ lanes, const uint32_t* __restrict__ segx, int nlanes,
                                                             ScanGeom g, int first, const unsigned long long* __restrict__ cur,
                                                             const uint32_t* __restrict__ cur_n, unsigned long long* __restrict__ nxt,
                                                             uint32_t* __restrict__ nxt_n, unsigned long long* __restrict__ entry,
                                                             uint32_t* __restrict__ flags) {
  __shared__ uint32_t tab[TABLE_WORDS];
  for (int i = threadIdx.x; i < TABLE_WORDS; i += JT) tab[i] = tables[i];
  __syncthreads();
  const int i = blockIdx.x * JT + threadIdx.x;
  if (i >= nlanes) return;
  const uint32_t start = lanes[3 * i], end = lanes[3 * i + 1], seg = lanes[3 * i + 2];
  const uint32_t seg_end = segx[4 * seg];
  const bool head = segx[4 * seg + 1] == (uint32_t)i;
  unsigned long long in;
  if (first) {
    in = (unsigned long long)start | ((unsigned long long)(AC ? g.ss : 0) << 32);
  } else {
    const unsigned long long mine = cur[i];
    const uint32_t mine_n = cur_n[i];
    if (head) { nxt[i] = mine; nxt_n[i] = mine_n; return; }
    in = cur[i - 1];
    if (in == entry[i]) { nxt[i] = mine; nxt_n[i] = mine_n; return; }
  }
  uint32_t p = (uint32_t)in, n = 0, blk = 0;
  int st = (int)((in >> 32) & 127u);
  prog_lane<AC, false>(scan, tab, g, p, st, n, end, seg_end, nullptr, nullptr, nullptr, blk, 0, nullptr);
  const unsigned long long out = (unsigned long long)p | ((unsigned long long)st << 32);
  entry[i] = in;
  nxt[i] = out;
  nxt_n[i] = n;
  if (!first && (out != cur[i] || n != cur_n[i])) atomicAdd(flags, 1u);
}

// exclusive saturating prefix sum of the lanes' block counts (one block; each thread sums a run of lanes, the runs are scanned in LDS)
__global__ __launch_bounds__(1024) void jpeg_prog_lane_scan_kernel(const uint32_t* __restrict__ count, int nlanes, uint32_t* __restrict__ prefix) {
  __shared__ uint32_t part[1024];
  const int t = threadIdx.x, per = (nlanes + 1023) / 1024;
  const int a = min(t * per, nlanes), e = min(a + per, nlanes);
  uint32_t sum = 0;
  for (int i = a; i < e; ++i) sum = sat_add(sum, count[i]);
  part[t] = sum;
  __syncthreads();
  for (int o = 1; o < 1024; o <<= 1) {
    const uint32_t v = t >= o ? part[t - o] : 0u;
    __syncthreads();
    part[t] = sat_add(part[t], v);
    __syncthreads();
  }
  uint32_t run = t > 0 ? part[t - 1] : 0u;
  for (int i = a; i < e; ++i) {
    prefix[i] = run;
    run = sat_add(run, count[i]);
  }
}

// the last pass: every lane decodes again from its true entry state and writes its blocks
template <bool AC>
__global__ __launch_bounds__(JT) void jpeg_prog_write_kernel(const uint32_t* __restrict__ scan, const uint32_t* __restrict__ tables,
                                                              const uint32_t* __restrict__ lanes, const uint32_t* __restrict__ segx, int nlanes,
                                                              ScanGeom g, const unsigned long long* __restrict__ state,
                                                              const uint32_t* __restrict__ prefix, int* __restrict__ diff, int16_t* __restrict__ coef,
                                                              const int32_t* __restrict__ map, uint32_t* __restrict__ flags) {
  __shared__ uint32_t tab[TABLE_WORDS];
  for (int i = threadIdx.x; i < TABLE_WORDS; i += JT) tab[i] = tables[i];
  __syncthreads();
  const int i = blockIdx.x * JT + threadIdx.x;
  if (i >= nlanes) return;
  const uint32_t start = lanes[3 * i], end = lanes[3 * i + 1], seg = lanes[3 * i + 2];
  const uint32_t seg_end = segx[4 * seg], head_lane = segx[4 * seg + 1], base = segx[4 * seg + 2], count = segx[4 * seg + 3];
  const int st0 = AC ? g.ss : 0;
  const unsigned long long in = head_lane == (uint32_t)i ? ((unsigned long long)start | ((unsigned long long)st0 << 32)) : state[i - 1];
  uint32_t p = (uint32_t)in, n = 0;
  int st = (int)((in >> 32) & 127u);
  // blocks the lanes before this one completed in the segment; the scan's walk holds base + count <= nblocks blocks
  const uint32_t before = prefix[i] >= prefix[head_lane] ? prefix[i] - prefix[head_lane] : COUNT_CAP;
  const uint32_t limit = min(base, (uint32_t)g.nblocks) + min(count, (uint32_t)g.nblocks - min(base, (uint32_t)g.nblocks));
  uint32_t blk = before < count ? base + before : limit;
  blk = min(blk, limit);
  prog_lane<AC, true>(scan, tab, g, p, st, n, end, seg_end, diff, coef, map, blk, limit, flags + 1);
  // the segment's last lane: the true final state must be a block's start after exactly the segment's blocks
  const bool tail = (i + 1 == nlanes) || lanes[3 * (i + 1) + 2] != seg;
  if (tail && (blk != limit || st != st0)) atomicOr(flags + 1, 4u);
}

// ---- DC differences (scan order) -> absolute DCs, shifted by Al, through the block map
__device__ __forceinline__ int dc_channel(const ScanGeom& g, int j) { return (g.comp_of >> (2 * ((j % g.segblocks) % g.bpu))) & 3; }
__global__ __launch_bounds__(JT) void jpeg_prog_dc_partial_kernel(ScanGeom g, const int* __restrict__ diff, int* __restrict__ local, Dc4* __restrict__ agg) {
  __shared__ Dc4 sh[JT];
  const int j = blockIdx.x * JT + threadIdx.x;
  Dc4 x = {0, 0, 0, 0};
  int c = 0;
  if (j < g.nblocks) {
    c = dc_channel(g, j);
    const int v = diff[j];
    x.f = (j % g.segblocks) == 0;
    x.v0 = c == 0 ? v : 0;
    x.v1 = c == 1 ? v : 0;
    x.v2 = c == 2 ? v : 0;
  }
  x = dc_block_scan(x, sh);
  if (j < g.nblocks) local[j] = c == 0 ? x.v0 : (c == 1 ? x.v1 : x.v2);
  if (threadIdx.x == JT - 1) agg[blockIdx.x] = x;
}
__global__ __launch_bounds__(JT) void jpeg_prog_dc_store_kernel(ScanGeom g, const int* __restrict__ local, const Dc4* __restrict__ carry,
                                                                 const int32_t* __restrict__ map, int16_t* __restrict__ coef) {
  const int j = blockIdx.x * JT + threadIdx.x;
  if (j >= g.nblocks) return;
  const int first = blockIdx.x * JT;
  const bool open = (first % g.segblocks) != 0 && (j / g.segblocks) == (first / g.segblocks);
  const int c = dc_channel(g, j);
  const Dc4 cr = carry[blockIdx.x];
  const int dc = local[j] + (open ? (c == 0 ? cr.v0 : (c == 1 ? cr.v1 : cr.v2)) : 0);
  coef[block_at(map, j) * 64] = (int16_t)(dc * (1 << g.al));
}

// DC refinement: bit i of a restart interval belongs to its block i
__global__ __launch_bounds__(JT) void jpeg_prog_dc_refine_kernel(ScanGeom g, const uint8_t* __restrict__ scan, long scan_bytes,
                                                                  const uint32_t* __restrict__ segs, const int32_t* __restrict__ map,
                                                                  int16_t* __restrict__ coef) {
  const int j = blockIdx.x * JT + threadIdx.x;
  if (j >= g.nblocks) return;
  const int seg = j / g.segblocks;
  const uint32_t at = segs[2 * seg] + (uint32_t)(j % g.segblocks);
  if (at >= segs[2 * seg + 1] || (long)(at >> 3) >= scan_bytes) return;
  if ((scan[at >> 3] >> (7 - (at & 7u))) & 1u) coef[block_at(map, j) * 64] |= (int16_t)(1 << g.al);
}

// the masks and records of AC refinement are in zigzag order: bit k = the coefficient at zigzag position k
__device__ const uint8_t ZZ_NATURAL[64] = {0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
__device__ const uint8_t ZZ_POSITION[64] = {0, 1, 5, 6, 14, 15, 27, 28, 2, 4, 7, 13, 16, 26, 29, 42, 3, 8, 12, 17, 25, 30, 41, 43, 9, 11, 18, 24, 31, 40, 44, 53, 10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38, 46, 51, 55, 60, 21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63};      // the inverse

// one thread per block of the component: bit k of the mask = the coefficient at zigzag position k is non-zero
__global__ __launch_bounds__(JT) void jpeg_prog_mask_kernel(int nblocks, const int16_t* __restrict__ coef, const int32_t* __restrict__ map,
                                                             unsigned long long* __restrict__ masks) {
  const int j = blockIdx.x * JT + threadIdx.x;
  if (j >= nblocks) return;
  const uint4* src = reinterpret_cast<const uint4*>(coef + block_at(map, j) * 64);
  unsigned long long m = 0;
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    const uint4 q = src[r];
    const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      m |= (unsigned long long)((w[i] & 0xffffu) != 0) << ZZ_POSITION[8 * r + 2 * i];
      m |= (unsigned long long)((w[i] >> 16) != 0) << ZZ_POSITION[8 * r + 2 * i + 1];
    }
  }
  masks[j] = m;
}

// one thread per zigzag position: the host's records {correction, new, sign of new} of an AC-refinement scan
__global__ __launch_bounds__(JT) void jpeg_prog_apply_kernel(int nblocks, int al, const unsigned long long* __restrict__ records,
                                                              const int32_t* __restrict__ map, int16_t* __restrict__ coef) {
  const long t = (long)blockIdx.x * JT + threadIdx.x;
  const int j = (int)(t >> 6), i = (int)(t & 63);
  if (j >= nblocks) return;
  const unsigned long long corr = records[3l * j], fresh = records[3l * j + 1], sign = records[3l * j + 2];
  if (!(((corr | fresh) >> i) & 1ull)) return;
  int16_t* c = coef + block_at(map, j) * 64 + ZZ_NATURAL[i];
  const int p1 = 1 << al, v = *c;
  *c = (int16_t)(((fresh >> i) & 1ull) ? (((sign >> i) & 1ull) ? -p1 : p1) : (v >= 0 ? v + p1 : v - p1));
}

// entropy workspace: flags (16 bytes) | state A | state B | entry (8 bytes per lane each) | count A | count B | prefix (4 per lane) |
// differences | DC local (4 per block of the scan) | DC aggregates (16 per chunk)
struct ProgWs {
  long flags, a, b, entry, na, nb, prefix, diff, local, agg, total;
  int nchunks;
  ProgWs(long nlanes, long nblocks) {
    nchunks = (int)((nblocks + JT - 1) / JT);
    flags = 0;
    a = 16;
    b = a + 8 * nlanes;
    entry = b + 8 * nlanes;
    na = entry + 8 * nlanes;
    nb = na + 4 * nlanes;
    prefix = nb + 4 * nlanes;
    diff = (prefix + 4 * nlanes + 15) & ~15l;
    local = (diff + 4 * nblocks + 15) & ~15l;
    agg = (local + 4 * nblocks + 15) & ~15l;
    total = agg + 16l * nchunks;
  }
};

ScanGeom scan_geom(const pf_jpeg_header* h, const pf_jpeg_prog_scan* sc) {
  ScanGeom g;
  g.ss = sc->ss; g.se = sc->se; g.al = sc->al; g.bpu = sc->blocks_per_unit; g.nblocks = sc->nblocks;
  g.segblocks = sc->restart_interval ? sc->restart_interval * sc->blocks_per_unit : sc->nblocks;
  g.comp_of = 0;
  if (sc->ncomp > 1) {
    int comp[6];
    block_components(h, comp);
    for (int b = 0; b < h->blocks_per_mcu; ++b) g.comp_of |= (uint32_t)comp[b] << (2 * b);
  }
  return g;
}

// a one-component scan needs its block map; an interleaved one walks the array itself
bool map_ok(const pf_jpeg_prog_scan* sc, const int32_t* map) { return (sc->ncomp > 1) == (map == nullptr); }

template <bool AC>
int decode_scan(const pf_jpeg_prog_scan* sc, const ScanGeom& g, const uint32_t* scan32, const uint32_t* lanes, const uint32_t* segx, int nlanes,
                int longest, const uint32_t* tables, const int32_t* map, int max_sync_rounds, uint8_t* ws, int16_t* coef, int* sync_rounds,
                hipStream_t s) {
  const ProgWs w(nlanes, sc->nblocks);
  uint32_t* flags = reinterpret_cast<uint32_t*>(ws + w.flags);
  unsigned long long* st[2] = {reinterpret_cast<unsigned long long*>(ws + w.a), reinterpret_cast<unsigned long long*>(ws + w.b)};
  uint32_t* cnt[2] = {reinterpret_cast<uint32_t*>(ws + w.na), reinterpret_cast<uint32_t*>(ws + w.nb)};
  unsigned long long* entry = reinterpret_cast<unsigned long long*>(ws + w.entry);
  uint32_t* prefix = reinterpret_cast<uint32_t*>(ws + w.prefix);
  int* diff = reinterpret_cast<int*>(ws + w.diff);
  const int grid = (nlanes + JT - 1) / JT;
  if (hipMemsetAsync(flags, 0, 16, s) != hipSuccess) return PF_ERR_LAUNCH;
  hipLaunchKernelGGL(jpeg_prog_sync_kernel<AC>, dim3(grid), dim3(JT), 0, s, scan32, tables, lanes, segx, nlanes, g, 1, st[1], cnt[1], st[0], cnt[0],
                     entry, flags);
  int cur = 0;
  // as in jpeg.hip: after r rounds every lane at most r places into its segment holds its true exit state
  for (int r = 1; r < longest; ++r) {
    if (r > max_sync_rounds) return pf_jpeg::NOT_CONVERGED;
    hipLaunchKernelGGL(jpeg_prog_sync_kernel<AC>, dim3(grid), dim3(JT), 0, s, scan32, tables, lanes, segx, nlanes, g, 0, st[cur], cnt[cur],
                       st[cur ^ 1], cnt[cur ^ 1], entry, flags);
    uint32_t changed = 0;
    if (hipMemcpyAsync(&changed, flags, sizeof(changed), hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
      return PF_ERR_LAUNCH;
    cur ^= 1;
    *sync_rounds = r;
    if (!changed) break;
    if (hipMemsetAsync(flags, 0, 4, s) != hipSuccess) return PF_ERR_LAUNCH;
  }
  hipLaunchKernelGGL(jpeg_prog_lane_scan_kernel, dim3(1), dim3(1024), 0, s, cnt[cur], nlanes, prefix);
  hipLaunchKernelGGL(jpeg_prog_write_kernel<AC>, dim3(grid), dim3(JT), 0, s, scan32, tables, lanes, segx, nlanes, g, st[cur], prefix, diff, coef, map,
                     flags);
  if (!AC) {
    int* local = reinterpret_cast<int*>(ws + w.local);
    Dc4* agg = reinterpret_cast<Dc4*>(ws + w.agg);
    hipLaunchKernelGGL(jpeg_prog_dc_partial_kernel, dim3(w.nchunks), dim3(JT), 0, s, g, diff, local, agg);
    hipLaunchKernelGGL(jpeg_dc_carry_kernel, dim3(1), dim3(JT), 0, s, agg, w.nchunks);
    hipLaunchKernelGGL(jpeg_prog_dc_store_kernel, dim3(w.nchunks), dim3(JT), 0, s, g, local, agg, map, coef);
  }
  uint32_t err = 0;
  if (hipMemcpyAsync(&err, flags + 1, sizeof(err), hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
    return PF_ERR_LAUNCH;
  if (ok() != PF_OK) return PF_ERR_LAUNCH;
  return err ? pf_jpeg::E_STREAM : PF_OK;
}

}  // namespace

// ---- host-only steps: no GPU call
extern "C" int pf_jpeg_prog_parse(const uint8_t* data, long len, pf_jpeg_header* header, pf_jpeg_prog_scan* scans, int scan_capacity, int* nscans) {
  return pf_jpeg::prog_parse(data, len, header, scans, scan_capacity, nscans);
}
extern "C" int pf_jpeg_prog_prepare_scan(const uint8_t* data, long len, const pf_jpeg_prog_scan* scan, uint8_t* out, long capacity, long* scan_bytes,
                                         uint32_t* segs) {
  return pf_jpeg::prog_prepare_scan(data, len, scan, out, capacity, scan_bytes, segs);
}
extern "C" int pf_jpeg_prog_decode_scan_host(const pf_jpeg_header* header, const pf_jpeg_prog_scan* scan, const uint8_t* bytes, long scan_bytes,
                                             const uint32_t* segs, int16_t* coef) {
  return pf_jpeg::prog_decode_scan(header, scan, bytes, scan_bytes, segs, coef);
}
extern "C" int pf_jpeg_prog_refine_ac_host(const pf_jpeg_prog_scan* scan, const uint8_t* bytes, long scan_bytes, const uint32_t* segs, uint64_t* masks,
                                           uint64_t* records) {
  return pf_jpeg::prog_refine_ac(scan, bytes, scan_bytes, segs, masks, records);
}
extern "C" int pf_jpeg_prog_plan(const pf_jpeg_prog_scan* scan, const uint32_t* segs, int subsequence_bits, uint32_t* lanes, long lane_capacity,
                                 uint32_t* segx, int* nlanes, int* longest) {
  return pf_jpeg::prog_plan(scan, segs, subsequence_bits, lanes, lane_capacity, segx, nlanes, longest);
}
extern "C" int pf_jpeg_prog_build_tables(const pf_jpeg_prog_scan* scan, uint32_t* tables) { return pf_jpeg::prog_build_tables(scan, tables); }
extern "C" int pf_jpeg_prog_block_map(const pf_jpeg_header* header, const pf_jpeg_prog_scan* scan, int32_t* map) {
  return pf_jpeg::prog_block_map(header, scan, map);
}
extern "C" int pf_jpeg_prog_workspace_bytes(int nlanes, int scan_blocks, long* bytes) {
  if (nlanes < 0 || scan_blocks < 1 || !bytes) return PF_ERR_ARG;
  *bytes = ProgWs(nlanes, scan_blocks).total;
  return PF_OK;
}

// ---- device steps
extern "C" int pf_jpeg_prog_decode_scan(const pf_jpeg_header* header, const pf_jpeg_prog_scan* scan, const uint8_t* bytes, long scan_bytes,
                                        const uint32_t* lanes, const uint32_t* segx, int nlanes, int longest, const uint32_t* tables,
                                        const int32_t* map, int max_sync_rounds, void* workspace, int16_t* coef, int* sync_rounds, void* stream) {
  if (!prog_scan_fits(header, scan) || (scan->kind != DC_FIRST && scan->kind != AC_FIRST) || !map_ok(scan, map)) return PF_ERR_ARG;
  if (!bytes || !lanes || !segx || !tables || !workspace || !coef || !sync_rounds || nlanes < scan->nsegments || longest < 1 || longest > nlanes ||
      max_sync_rounds < 0 || scan_bytes < SCAN_PAD)
    return PF_ERR_ARG;
  if ((reinterpret_cast<uintptr_t>(workspace) & 15u) || (reinterpret_cast<uintptr_t>(bytes) & 3u) || (reinterpret_cast<uintptr_t>(coef) & 15u))
    return PF_ERR_ARG;
  *sync_rounds = 0;
  const ScanGeom g = scan_geom(header, scan);
  const uint32_t* scan32 = reinterpret_cast<const uint32_t*>(bytes);
  uint8_t* ws = static_cast<uint8_t*>(workspace);
  if (scan->kind == AC_FIRST)
    return decode_scan<true>(scan, g, scan32, lanes, segx, nlanes, longest, tables, map, max_sync_rounds, ws, coef, sync_rounds, ST(stream));
  return decode_scan<false>(scan, g, scan32, lanes, segx, nlanes, longest, tables, map, max_sync_rounds, ws, coef, sync_rounds, ST(stream));
}

extern "C" int pf_jpeg_prog_dc_refine(const pf_jpeg_header* header, const pf_jpeg_prog_scan* scan, const uint8_t* bytes, long scan_bytes,
                                      const uint32_t* segs, const int32_t* map, int16_t* coef, void* stream) {
  if (!prog_scan_fits(header, scan) || scan->kind != DC_REFINE || !map_ok(scan, map) || !bytes || !segs || !coef || scan_bytes < SCAN_PAD)
    return PF_ERR_ARG;
  const ScanGeom g = scan_geom(header, scan);
  hipLaunchKernelGGL(jpeg_prog_dc_refine_kernel, dim3((g.nblocks + JT - 1) / JT), dim3(JT), 0, ST(stream), g, bytes, scan_bytes, segs, map, coef);
  return ok();
}

extern "C" int pf_jpeg_prog_nonzero_mask(const pf_jpeg_header* header, const pf_jpeg_prog_scan* scan, const int16_t* coef, const int32_t* map,
                                         uint64_t* masks, void* stream) {
  if (!prog_scan_fits(header, scan) || !map_ok(scan, map) || !coef || !masks || (reinterpret_cast<uintptr_t>(coef) & 15u)) return PF_ERR_ARG;
  hipLaunchKernelGGL(jpeg_prog_mask_kernel, dim3((scan->nblocks + JT - 1) / JT), dim3(JT), 0, ST(stream), scan->nblocks, coef, map,
                     reinterpret_cast<unsigned long long*>(masks));
  return ok();
}

extern "C" int pf_jpeg_prog_apply_refinement(const pf_jpeg_header* header, const pf_jpeg_prog_scan* scan, const uint64_t* records, const int32_t* map,
                                             int16_t* coef, void* stream) {
  if (!prog_scan_fits(header, scan) || scan->kind != AC_REFINE || !map_ok(scan, map) || !records || !coef) return PF_ERR_ARG;
  const long threads = (long)scan->nblocks * 64;
  hipLaunchKernelGGL(jpeg_prog_apply_kernel, dim3((unsigned)((threads + JT - 1) / JT)), dim3(JT), 0, ST(stream), scan->nblocks, scan->al,
                     reinterpret_cast<const unsigned long long*>(records), map, coef);
  return ok();
}
