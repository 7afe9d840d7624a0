// Baseline JPEG decoding on the device (include/pf_hip.h, "JPEG decoding"): the entropy decoder over self-synchronising subsequences
// (Weissenberger and Schmidt, ICPP 2018) and libjpeg's integer reconstruction (jidctint.c islow, jdsample.c fancy upsampling, jdcolor.c).
// Marker parsing, scan preparation, the subsequence plan and the decode tables are host code (jpeg_host.h).
//
// Entropy decoder.  A lane owns one subsequence [start, end) of a restart interval ("segment").  Its decoder state is (p, b, k): bit
// position, block inside the MCU, zigzag position (0 = a DC code comes next).  The first lane of a segment starts from the known state
// (segment start, 0, 0); every other lane first guesses (its own start, 0, 0) and is then re-decoded from the exit state of the lane
// before it until a round changes no exit state.  Exit states are double-buffered, so a round reads only the states of the round before:
// the number of rounds is a property of the file and of S, not of the schedule.  A lane whose entry state did not change is not re-decoded.
//
// Termination and bounds (the invariants every kernel below keeps):
//   * every decoder step consumes at least one bit or leaves the loop: a code that matches no table entry consumes one bit and sets nothing;
//   * a symbol that would run past its segment's end ends the lane (the state stays in front of that symbol);
//   * every decode loop runs while p < end, so it is bounded by S plus one symbol (a lane entered in front of its start, which only
//     happens within one symbol of a segment's end, by S plus two);
//   * k is clamped to 63 before it indexes the zigzag table;
//   * a coefficient is written only for a block index below its segment's first block + block count, which lies inside the array;
//   * every 64-bit window read lies inside the scan buffer: p < segment end <= 8 * (scan_bytes - SCAN_PAD);
//   * the host's round loop is bounded by the longest segment in lanes and by max_sync_rounds.
#include "pf_common.h"
#include "../../include/pf_hip.h"
#include "jpeg_host.h"
#include "jpeg_dev.h"

namespace {

using namespace pf_jpeg;

// exit state of a lane in one word, so that a lane reads its neighbour's state whole: p | k << 32 | b << 39 | blocks << 42
__device__ __forceinline__ unsigned long long pack_state(uint32_t p, int b, int k, uint32_t n) {
  return (unsigned long long)p | ((unsigned long long)k << 32) | ((unsigned long long)b << 39) | ((unsigned long long)n << 42);
}
constexpr unsigned long long STATE_MASK = (1ull << 42) - 1;      // (p, b, k) without the block count

// Decodes from (p, b, k) while p < end.  WRITE: coefficients go to coef for blocks [blk, limit), DC differences in slot 0; the lane stops
// at blk == limit, and an invalid code or more than 7 bits left over at that point raise *err.
template <bool WRITE>
__device__ __forceinline__ void decode_lane(const uint32_t* __restrict__ scan, const uint32_t* tab, int bpm, uint32_t comp_of, uint32_t& p, int& b,
                                            int& k, uint32_t& n, uint32_t end, uint32_t seg_end, int16_t* __restrict__ coef, uint32_t blk,
                                            uint32_t limit, uint32_t* err) {
  const uint8_t* zz = reinterpret_cast<const uint8_t*>(tab + T_ZIGZAG);
  uint32_t wi = 0xffffffffu, hi = 0, lo = 0;          // the two scan words around p, in bit order (the scan is written big-endian)
  while (p < end) {
    if (WRITE && blk >= limit) break;
    if ((p >> 5) != wi) {
      wi = p >> 5;
      hi = __builtin_bswap32(scan[wi]);
      lo = __builtin_bswap32(scan[wi + 1]);
    }
    const uint32_t win = (p & 31u) ? (hi << (p & 31u)) | (lo >> (32u - (p & 31u))) : hi;      // the 32 bits from p on
    const uint32_t* T = tab + (2 * ((comp_of >> (2 * b)) & 3u) + (k != 0)) * T_WORDS;
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
    const bool valid = len != 0;        // no such code: one bit consumed, nothing set
    if (!valid) {
      if (WRITE) atomicOr(err, 1u);
      len = 1;
      sym = 0;
    }
    const uint32_t s = sym & 15u, r = k ? (sym >> 4) : 0u;
    if (p + len + s > seg_end) break;   // the symbol runs past the segment: the lane ends in front of it
    const uint32_t bits = s ? ((win << len) >> (32u - s)) : 0u;       // len + s <= 31
    const int val = s ? (bits < (1u << (s - 1)) ? (int)bits - (1 << s) + 1 : (int)bits) : 0;
    p += len + s;
    if (!valid) continue;
    if (k == 0) {
      if (WRITE) coef[(long)blk * 64] = (int16_t)val;
      k = 1;
    } else if (s == 0) {
      k = (r == 15u) ? k + 16 : 64;
    } else {
      k += (int)r;
      if (WRITE) coef[(long)blk * 64 + zz[k < 63 ? k : 63]] = (int16_t)val;
      ++k;
    }
    if (k >= 64) {
      k = 0;
      b = (b + 1 == bpm) ? 0 : b + 1;
      ++n;
      ++blk;
      if (WRITE && blk == limit && seg_end - p > 7u) atomicOr(err, 2u);
    }
  }
}

// round 0 (first != 0): every lane from (its start, 0, 0).  Later rounds: every lane that is not the first of its segment from the
// exit state `cur` holds for the lane before it; flags[0] counts the exit states that changed.
__global__ __launch_bounds__(JT) void jpeg_sync_kernel(const uint32_t* __restrict__ scan, const uint32_t* __restrict__ tables,
                                                        const uint32_t* __restrict__ lanes, const uint32_t* __restrict__ segx, int nlanes, int bpm,
                                                        uint32_t comp_of, int first, const unsigned long long* __restrict__ cur,
                                                        unsigned long long* __restrict__ nxt, unsigned long long* __restrict__ entry,
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
    in = pack_state(start, 0, 0, 0);
  } else {
    const unsigned long long mine = cur[i];
    if (head) { nxt[i] = mine; return; }
    in = cur[i - 1] & STATE_MASK;
    if (in == entry[i]) { nxt[i] = mine; return; }
  }
  uint32_t p = (uint32_t)in, n = 0;
  int k = (int)((in >> 32) & 127u), b = (int)((in >> 39) & 7u);
  decode_lane<false>(scan, tab, bpm, comp_of, p, b, k, n, end, seg_end, nullptr, 0, 0, nullptr);
  const unsigned long long out = pack_state(p, b, k, n);
  entry[i] = in;
  nxt[i] = out;
  if (!first && out != cur[i]) atomicAdd(flags, 1u);
}

// exclusive prefix sum of the lanes' block counts (one block; each thread sums a run of lanes, the runs are scanned in LDS)
__global__ __launch_bounds__(1024) void jpeg_lane_scan_kernel(const unsigned long long* __restrict__ state, int nlanes, uint32_t* __restrict__ prefix) {
  __shared__ uint32_t part[1024];
  const int t = threadIdx.x, per = (nlanes + 1023) / 1024;
  const int a = min(t * per, nlanes), e = min(a + per, nlanes);
  uint32_t sum = 0;
  for (int i = a; i < e; ++i) sum += (uint32_t)(state[i] >> 42);
  part[t] = sum;
  __syncthreads();
  for (int o = 1; o < 1024; o <<= 1) {
    const uint32_t v = t >= o ? part[t - o] : 0u;
    __syncthreads();
    part[t] += v;
    __syncthreads();
  }
  uint32_t run = part[t] - sum;
  for (int i = a; i < e; ++i) {
    prefix[i] = run;
    run += (uint32_t)(state[i] >> 42);
  }
}

// the last pass: every lane decodes again from its true entry state and writes its blocks
__global__ __launch_bounds__(JT) void jpeg_write_kernel(const uint32_t* __restrict__ scan, const uint32_t* __restrict__ tables,
                                                         const uint32_t* __restrict__ lanes, const uint32_t* __restrict__ segx, int nlanes, int bpm,
                                                         uint32_t comp_of, const unsigned long long* __restrict__ state,
                                                         const uint32_t* __restrict__ prefix, int16_t* __restrict__ coef, uint32_t* __restrict__ flags) {
  __shared__ uint32_t tab[TABLE_WORDS];
  for (int i = threadIdx.x; i < TABLE_WORDS; i += JT) tab[i] = tables[i];
  __syncthreads();
  const int i = blockIdx.x * JT + threadIdx.x;
  if (i >= nlanes) return;
  const uint32_t start = lanes[3 * i], end = lanes[3 * i + 1], seg = lanes[3 * i + 2];
  const uint32_t seg_end = segx[4 * seg], head_lane = segx[4 * seg + 1], base = segx[4 * seg + 2], count = segx[4 * seg + 3];
  const bool head = head_lane == (uint32_t)i;
  const unsigned long long in = head ? pack_state(start, 0, 0, 0) : (state[i - 1] & STATE_MASK);
  uint32_t p = (uint32_t)in, n = 0;
  int k = (int)((in >> 32) & 127u), b = (int)((in >> 39) & 7u);
  const uint32_t done = prefix[i] - prefix[head_lane];              // blocks the lanes before this one completed in the segment
  const uint32_t limit = base + count;
  const uint32_t blk = done < count ? base + done : limit;
  decode_lane<true>(scan, tab, bpm, comp_of, p, b, k, n, end, seg_end, coef, blk, limit, flags + 1);
  // the segment's last lane: the true final state must be (k = 0, b = 0, blocks = expected)
  const bool tail = (i + 1 == nlanes) || lanes[3 * (i + 1) + 2] != seg;
  if (tail && blk + n != limit) atomicOr(flags + 1, 4u);
}

// ---- DC differences -> absolute DCs: a segmented scan over the blocks, one channel per component.  Segments start at multiples of segblocks.
struct DcGeom {
  int nblocks, bpm, segblocks;      // segblocks = restart interval * bpm, or nblocks without restart intervals
  uint32_t comp_of;
};
__device__ __forceinline__ Dc4 dc_element(const DcGeom& g, const int16_t* __restrict__ coef, int j) {
  Dc4 x = {0, 0, 0, 0};
  if (j < g.nblocks) {
    const int c = (g.comp_of >> (2 * ((j % g.segblocks) % g.bpm))) & 3, v = coef[(long)j * 64];
    x.f = (j % g.segblocks) == 0;
    x.v0 = c == 0 ? v : 0;
    x.v1 = c == 1 ? v : 0;
    x.v2 = c == 2 ? v : 0;
  }
  return x;
}
// per chunk of JT blocks: the inclusive scan inside the chunk (own component's channel -> local) and the chunk's aggregate
__global__ __launch_bounds__(JT) void jpeg_dc_partial_kernel(DcGeom g, const int16_t* __restrict__ coef, int* __restrict__ local, Dc4* __restrict__ agg) {
  __shared__ Dc4 sh[JT];
  const int j = blockIdx.x * JT + threadIdx.x;
  const Dc4 x = dc_block_scan(dc_element(g, coef, j), sh);
  if (j < g.nblocks) {
    const int c = (g.comp_of >> (2 * ((j % g.segblocks) % g.bpm))) & 3;
    local[j] = c == 0 ? x.v0 : (c == 1 ? x.v1 : x.v2);
  }
  if (threadIdx.x == JT - 1) agg[blockIdx.x] = x;
}
__global__ __launch_bounds__(JT) void jpeg_dc_apply_kernel(DcGeom g, const int* __restrict__ local, const Dc4* __restrict__ carry, int16_t* __restrict__ coef) {
  const int j = blockIdx.x * JT + threadIdx.x;
  if (j >= g.nblocks) return;
  const int first = blockIdx.x * JT;
  // the carry of the chunks before applies while no segment has started inside this chunk up to j
  const bool open = (first % g.segblocks) != 0 && (j / g.segblocks) == (first / g.segblocks);
  const int c = (g.comp_of >> (2 * ((j % g.segblocks) % g.bpm))) & 3;
  const Dc4 cr = carry[blockIdx.x];
  coef[(long)j * 64] = (int16_t)(local[j] + (open ? (c == 0 ? cr.v0 : (c == 1 ? cr.v1 : cr.v2)) : 0));
}

// ------------------------------------------------------------------------------------------------ reconstruction
struct ReconGeom {
  int W, H, ncomp, hmax, vmax, mcus_x, nblocks, bpm, orientation;
  int blk_comp[6], blk_h[6], blk_v[6];
  int comp_h[3], comp_v[3];         // blocks per MCU across / down
  int plane_w[3], plane_h[3];       // padded to whole MCUs
  long plane_off[3];
  int samp_w[3], samp_h[3];         // the component's downsampled size: ceil(W * h / hmax), ceil(H * v / vmax)
  uint8_t qt[3][64];
};

#define FIX_0_298631336 2446
#define FIX_0_390180644 3196
#define FIX_0_541196100 4433
#define FIX_0_765366865 6270
#define FIX_0_899976223 7373
#define FIX_1_175875602 9633
#define FIX_1_501321110 12299
#define FIX_1_847759065 15137
#define FIX_1_961570560 16069
#define FIX_2_053119869 16819
#define FIX_2_562915447 20995
#define FIX_3_072711026 25172

// jpeg_idct_islow's one-dimensional pass on eight values; the caller descales.  32-bit arithmetic, as libjpeg-turbo's SIMD code; libjpeg's C
// code holds these sums in a 64-bit JLONG.  Every coefficient an encoder can produce from 8-bit samples stays far inside 32 bits (|dequantised|
// <= 2^11 * 8, times constants < 2^15, eight terms); a hostile stream (int16 coefficient x 255) can overflow, which wraps harmlessly here
// and then differs from the C library's result for that block.
__device__ __forceinline__ void idct8(const int (&in)[8], int (&out)[8]) {
  int z2 = in[2], z3 = in[6];
  int z1 = (z2 + z3) * FIX_0_541196100;
  int tmp2 = z1 + z3 * (-FIX_1_847759065);
  int tmp3 = z1 + z2 * FIX_0_765366865;
  z2 = in[0];
  z3 = in[4];
  int tmp0 = (z2 + z3) * 8192, tmp1 = (z2 - z3) * 8192;
  const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
  tmp0 = in[7];
  tmp1 = in[5];
  tmp2 = in[3];
  tmp3 = in[1];
  z1 = tmp0 + tmp3;
  z2 = tmp1 + tmp2;
  z3 = tmp0 + tmp2;
  int z4 = tmp1 + tmp3;
  const int z5 = (z3 + z4) * FIX_1_175875602;
  tmp0 *= FIX_0_298631336;
  tmp1 *= FIX_2_053119869;
  tmp2 *= FIX_3_072711026;
  tmp3 *= FIX_1_501321110;
  z1 *= -FIX_0_899976223;
  z2 *= -FIX_2_562915447;
  z3 *= -FIX_1_961570560;
  z4 *= -FIX_0_390180644;
  z3 += z5;
  z4 += z5;
  tmp0 += z1 + z3;
  tmp1 += z2 + z4;
  tmp2 += z2 + z3;
  tmp3 += z1 + z4;
  out[0] = tmp10 + tmp3;
  out[7] = tmp10 - tmp3;
  out[1] = tmp11 + tmp2;
  out[6] = tmp11 - tmp2;
  out[2] = tmp12 + tmp1;
  out[5] = tmp12 - tmp1;
  out[3] = tmp13 + tmp0;
  out[4] = tmp13 - tmp0;
}

// one thread per 8 x 8 block: dequantise, column pass (descale 11), row pass (descale 18), + 128, clamp, into the component's plane
__global__ __launch_bounds__(JT) void jpeg_idct_kernel(ReconGeom g, const int16_t* __restrict__ coef, uint8_t* __restrict__ planes) {
  __shared__ uint8_t qt[3][64];
  if (threadIdx.x < 192) qt[threadIdx.x >> 6][threadIdx.x & 63] = g.qt[threadIdx.x >> 6][threadIdx.x & 63];
  __syncthreads();
  const int j = blockIdx.x * JT + threadIdx.x;
  if (j >= g.nblocks) return;
  const int mcu = j / g.bpm, b = j - mcu * g.bpm, c = g.blk_comp[b];
  const int my = mcu / g.mcus_x, mx = mcu - my * g.mcus_x;
  const int bx = mx * g.comp_h[c] + g.blk_h[b], by = my * g.comp_v[c] + g.blk_v[b];
  int ws[64];
  const uint4* src = reinterpret_cast<const uint4*>(coef + (long)j * 64);
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    const uint4 q = src[r];
    const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      ws[8 * r + 2 * i] = (int)(int16_t)(w[i] & 0xffffu) * (int)qt[c][8 * r + 2 * i];
      ws[8 * r + 2 * i + 1] = (int)(int16_t)(w[i] >> 16) * (int)qt[c][8 * r + 2 * i + 1];
    }
  }
#pragma unroll
  for (int col = 0; col < 8; ++col) {
    int in[8], out[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) in[r] = ws[8 * r + col];
    idct8(in, out);
#pragma unroll
    for (int r = 0; r < 8; ++r) ws[8 * r + col] = (out[r] + (1 << 10)) >> 11;
  }
  uint8_t* dst = planes + g.plane_off[c] + (long)(by * 8) * g.plane_w[c] + bx * 8;
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    int in[8], out[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) in[i] = ws[8 * r + i];
    idct8(in, out);
    uint32_t px[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) px[i] = (uint32_t)min(max(((out[i] + (1 << 17)) >> 18) + 128, 0), 255);
    *reinterpret_cast<uint2*>(dst + (long)r * g.plane_w[c]) =
        make_uint2(px[0] | (px[1] << 8) | (px[2] << 16) | (px[3] << 24), px[4] | (px[5] << 8) | (px[6] << 16) | (px[7] << 24));
  }
}

// jdsample.c's fancy upsampling of one chroma sample at output pixel (x, y); edges replicate at the downsampled size (sw, sh)
__device__ __forceinline__ int upsample(const uint8_t* __restrict__ pl, int pw, int sw, int sh, int hs, int vs, int x, int y) {
  if (hs == 1) return pl[(long)y * pw + x];
  const int c = x >> 1;
  if (vs == 1) {                                          // h2v1
    const uint8_t* row = pl + (long)y * pw;
    const int t = row[c];
    if (x & 1) return c == sw - 1 ? t : (3 * t + row[c + 1] + 2) >> 2;
    return c == 0 ? t : (3 * t + row[c - 1] + 1) >> 2;
  }
  const int r = y >> 1;                                   // h2v2
  const int rn = (y & 1) ? min(r + 1, sh - 1) : max(r - 1, 0);
  const uint8_t *r0 = pl + (long)r * pw, *r1 = pl + (long)rn * pw;
  const int t = 3 * r0[c] + r1[c];
  if (x & 1) return c == sw - 1 ? (4 * t + 7) >> 4 : (3 * t + 3 * r0[c + 1] + r1[c + 1] + 7) >> 4;
  return c == 0 ? (4 * t + 8) >> 4 : (3 * t + 3 * r0[c - 1] + r1[c - 1] + 8) >> 4;
}

// one thread per pixel: upsample, jdcolor.c's YCbCr -> RGB (SCALEBITS 16), store at the orientation's address
__global__ __launch_bounds__(JT) void jpeg_color_store_kernel(ReconGeom g, const uint8_t* __restrict__ planes, uint8_t* __restrict__ out) {
  const int x = blockIdx.x * JT + threadIdx.x, y = blockIdx.y;
  if (x >= g.W) return;
  const int Y = planes[g.plane_off[0] + (long)y * g.plane_w[0] + x];
  int R = Y, G = Y, B = Y;
  if (g.ncomp == 3) {
    const int cb = upsample(planes + g.plane_off[1], g.plane_w[1], g.samp_w[1], g.samp_h[1], g.hmax, g.vmax, x, y) - 128;
    const int cr = upsample(planes + g.plane_off[2], g.plane_w[2], g.samp_w[2], g.samp_h[2], g.hmax, g.vmax, x, y) - 128;
    R = min(max(Y + ((91881 * cr + 32768) >> 16), 0), 255);
    G = min(max(Y + ((-22554 * cb - 46802 * cr + 32768) >> 16), 0), 255);
    B = min(max(Y + ((116130 * cb + 32768) >> 16), 0), 255);
  }
  int ox = x, oy = y, ow = g.W;
  switch (g.orientation) {
    case 2: ox = g.W - 1 - x; break;
    case 3: ox = g.W - 1 - x; oy = g.H - 1 - y; break;
    case 4: oy = g.H - 1 - y; break;
    case 5: ox = y; oy = x; ow = g.H; break;
    case 6: ox = g.H - 1 - y; oy = x; ow = g.H; break;
    case 7: ox = g.H - 1 - y; oy = g.W - 1 - x; ow = g.H; break;
    case 8: ox = y; oy = g.W - 1 - x; ow = g.H; break;
    default: break;
  }
  uint8_t* d = out + ((long)oy * ow + ox) * 3;
  d[0] = (uint8_t)R;
  d[1] = (uint8_t)G;
  d[2] = (uint8_t)B;
}

// ------------------------------------------------------------------------------------------------ host
bool header_ok(const pf_jpeg_header* h) {
  if (!h || h->width < 1 || h->height < 1 || (h->ncomp != 1 && h->ncomp != 3) || h->nblocks < 1 || h->nsegments < 1) return false;
  if (h->blocks_per_mcu < 1 || h->blocks_per_mcu > 6 || h->hmax < 1 || h->hmax > 2 || h->vmax < 1 || h->vmax > 2) return false;
  int bpm = 0;
  for (int c = 0; c < h->ncomp; ++c) {
    if (h->comp_h[c] < 1 || h->comp_h[c] > h->hmax || h->comp_v[c] < 1 || h->comp_v[c] > h->vmax || h->comp_tq[c] < 0 || h->comp_tq[c] > 3) return false;
    bpm += h->comp_h[c] * h->comp_v[c];
  }
  if (bpm != h->blocks_per_mcu || h->mcus_x != (h->width + 8 * h->hmax - 1) / (8 * h->hmax) ||
      h->mcus_y != (h->height + 8 * h->vmax - 1) / (8 * h->vmax) || (long)h->mcus_x * h->mcus_y * bpm != h->nblocks)
    return false;
  if (h->restart_interval < 0 || h->nsegments != (h->restart_interval ? ((long)h->mcus_x * h->mcus_y + h->restart_interval - 1) / h->restart_interval : 1))
    return false;
  return true;
}

uint32_t comp_of_word(const pf_jpeg_header* h) {
  int comp[6];
  block_components(h, comp);
  uint32_t w = 0;
  for (int b = 0; b < h->blocks_per_mcu; ++b) w |= (uint32_t)comp[b] << (2 * b);
  return w;
}

// entropy workspace: flags (4 words, 16 bytes) | state A | state B | entry (8 bytes per lane each) | prefix (4 per lane) | DC local (4 per
// block) | DC aggregates (16 per chunk)
struct EntropyWs {
  long flags, a, b, entry, prefix, local, agg, total;
  int nchunks;
  EntropyWs(long nlanes, long nblocks) {
    nchunks = (int)((nblocks + JT - 1) / JT);
    flags = 0;
    a = 16;
    b = a + 8 * nlanes;
    entry = b + 8 * nlanes;
    prefix = entry + 8 * nlanes;
    local = (prefix + 4 * nlanes + 15) & ~15l;
    agg = (local + 4 * nblocks + 15) & ~15l;
    total = agg + 16l * nchunks;
  }
};

void recon_geom(const pf_jpeg_header* h, int orientation, ReconGeom* g) {
  memset(g, 0, sizeof(*g));
  g->W = h->width; g->H = h->height; g->ncomp = h->ncomp; g->hmax = h->hmax; g->vmax = h->vmax; g->mcus_x = h->mcus_x;
  g->nblocks = h->nblocks; g->bpm = h->blocks_per_mcu; g->orientation = orientation;
  int b = 0;
  long off = 0;
  for (int c = 0; c < h->ncomp; ++c) {
    for (int v = 0; v < h->comp_v[c]; ++v)
      for (int x = 0; x < h->comp_h[c]; ++x) { g->blk_comp[b] = c; g->blk_h[b] = x; g->blk_v[b] = v; ++b; }
    g->comp_h[c] = h->comp_h[c]; g->comp_v[c] = h->comp_v[c];
    g->plane_w[c] = h->mcus_x * h->comp_h[c] * 8;
    g->plane_h[c] = h->mcus_y * h->comp_v[c] * 8;
    g->plane_off[c] = off;
    off += ((long)g->plane_w[c] * g->plane_h[c] + 15) & ~15l;
    g->samp_w[c] = (h->width * h->comp_h[c] + h->hmax - 1) / h->hmax;
    g->samp_h[c] = (h->height * h->comp_v[c] + h->vmax - 1) / h->vmax;
    memcpy(g->qt[c], h->qt[h->comp_tq[c]], 64);
  }
}

}  // namespace

// ---- host-only steps: no GPU call
extern "C" int pf_jpeg_parse(const uint8_t* data, long len, pf_jpeg_header* header) { return pf_jpeg::parse(data, len, header); }
extern "C" int pf_jpeg_prepare_scan(const uint8_t* data, long len, const pf_jpeg_header* header, uint8_t* scan, long scan_capacity,
                                    long* scan_bytes, uint32_t* segs) {
  return pf_jpeg::prepare_scan(data, len, header, scan, scan_capacity, scan_bytes, segs);
}
extern "C" int pf_jpeg_decode_entropy_host(const pf_jpeg_header* header, const uint8_t* scan, long scan_bytes, const uint32_t* segs, int16_t* coef) {
  if (!header_ok(header)) return PF_ERR_ARG;
  return pf_jpeg::decode_entropy(header, scan, scan_bytes, segs, coef);
}
extern "C" int pf_jpeg_plan(const pf_jpeg_header* header, const uint32_t* segs, int subsequence_bits, uint32_t* lanes, long lane_capacity,
                            uint32_t* segx, int* nlanes, int* longest) {
  if (!header_ok(header)) return PF_ERR_ARG;
  return pf_jpeg::plan(header, segs, subsequence_bits, lanes, lane_capacity, segx, nlanes, longest);
}
extern "C" int pf_jpeg_build_tables(const pf_jpeg_header* header, uint32_t* tables) {
  if (!header_ok(header)) return PF_ERR_ARG;
  return pf_jpeg::build_tables(header, tables);
}

// ---- device steps
extern "C" int pf_jpeg_workspace_bytes(const pf_jpeg_header* header, int nlanes, long* entropy_bytes, long* recon_bytes) {
  if (!header_ok(header) || nlanes < 0 || !entropy_bytes || !recon_bytes) return PF_ERR_ARG;
  *entropy_bytes = EntropyWs(nlanes, header->nblocks).total;
  ReconGeom g;
  recon_geom(header, 1, &g);
  const int last = header->ncomp - 1;
  *recon_bytes = g.plane_off[last] + (((long)g.plane_w[last] * g.plane_h[last] + 15) & ~15l);
  return PF_OK;
}

extern "C" int pf_jpeg_decode_entropy(const pf_jpeg_header* header, const uint8_t* scan, long scan_bytes, const uint32_t* lanes,
                                      const uint32_t* segx, int nlanes, int longest, const uint32_t* tables, int max_sync_rounds,
                                      void* workspace, int16_t* coef, int* sync_rounds, void* stream) {
  if (!header_ok(header) || !scan || !lanes || !segx || !tables || !workspace || !coef || !sync_rounds || nlanes < header->nsegments ||
      longest < 1 || longest > nlanes || max_sync_rounds < 0 || scan_bytes < SCAN_PAD)
    return PF_ERR_ARG;
  if ((reinterpret_cast<uintptr_t>(workspace) & 15u) || (reinterpret_cast<uintptr_t>(scan) & 3u) || (reinterpret_cast<uintptr_t>(coef) & 15u))
    return PF_ERR_ARG;
  const EntropyWs w(nlanes, header->nblocks);
  uint8_t* ws = static_cast<uint8_t*>(workspace);
  uint32_t* flags = reinterpret_cast<uint32_t*>(ws + w.flags);
  unsigned long long* st[2] = {reinterpret_cast<unsigned long long*>(ws + w.a), reinterpret_cast<unsigned long long*>(ws + w.b)};
  unsigned long long* entry = reinterpret_cast<unsigned long long*>(ws + w.entry);
  uint32_t* prefix = reinterpret_cast<uint32_t*>(ws + w.prefix);
  const uint32_t* scan32 = reinterpret_cast<const uint32_t*>(scan);
  const int bpm = header->blocks_per_mcu;
  const uint32_t comp_of = comp_of_word(header);
  const int grid = (nlanes + JT - 1) / JT;
  hipStream_t s = ST(stream);
  *sync_rounds = 0;
  if (hipMemsetAsync(flags, 0, 16, s) != hipSuccess) return PF_ERR_LAUNCH;
  if (hipMemsetAsync(coef, 0, (size_t)header->nblocks * 64 * sizeof(int16_t), s) != hipSuccess) return PF_ERR_LAUNCH;
  hipLaunchKernelGGL(jpeg_sync_kernel, dim3(grid), dim3(JT), 0, s, scan32, tables, lanes, segx, nlanes, bpm, comp_of, 1, st[1], st[0], entry, flags);
  int cur = 0;
  // After r rounds every lane at most r places into its segment holds its true exit state, so longest - 1 rounds always suffice; a round
  // that changes nothing ends the loop earlier.
  for (int r = 1; r < longest; ++r) {
    // (returns with the rounds so far still queued on the stream: the caller's buffers must stay alive in stream order, as torch's do)
    if (r > max_sync_rounds) return pf_jpeg::NOT_CONVERGED;
    hipLaunchKernelGGL(jpeg_sync_kernel, dim3(grid), dim3(JT), 0, s, scan32, tables, lanes, segx, nlanes, bpm, comp_of, 0, st[cur], st[cur ^ 1],
                       entry, flags);
    uint32_t changed = 0;
    if (hipMemcpyAsync(&changed, flags, sizeof(changed), hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
      return PF_ERR_LAUNCH;
    cur ^= 1;
    *sync_rounds = r;
    if (!changed) break;
    if (hipMemsetAsync(flags, 0, 4, s) != hipSuccess) return PF_ERR_LAUNCH;
  }
  hipLaunchKernelGGL(jpeg_lane_scan_kernel, dim3(1), dim3(1024), 0, s, st[cur], nlanes, prefix);
  hipLaunchKernelGGL(jpeg_write_kernel, dim3(grid), dim3(JT), 0, s, scan32, tables, lanes, segx, nlanes, bpm, comp_of, st[cur], prefix, coef, flags);
  DcGeom dg = {header->nblocks, bpm, header->restart_interval ? header->restart_interval * bpm : header->nblocks, comp_of};
  int* local = reinterpret_cast<int*>(ws + w.local);
  Dc4* agg = reinterpret_cast<Dc4*>(ws + w.agg);
  hipLaunchKernelGGL(jpeg_dc_partial_kernel, dim3(w.nchunks), dim3(JT), 0, s, dg, coef, local, agg);
  hipLaunchKernelGGL(jpeg_dc_carry_kernel, dim3(1), dim3(JT), 0, s, agg, w.nchunks);
  hipLaunchKernelGGL(jpeg_dc_apply_kernel, dim3(w.nchunks), dim3(JT), 0, s, dg, local, agg, coef);
  uint32_t err = 0;
  if (hipMemcpyAsync(&err, flags + 1, sizeof(err), hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
    return PF_ERR_LAUNCH;
  if (ok() != PF_OK) return PF_ERR_LAUNCH;
  return err ? pf_jpeg::E_STREAM : PF_OK;
}

extern "C" int pf_jpeg_reconstruct(const pf_jpeg_header* header, const int16_t* coef, int orientation, void* workspace, uint8_t* rgb, void* stream) {
  if (!header_ok(header) || !coef || !workspace || !rgb || orientation < 1 || orientation > 8) return PF_ERR_ARG;
  if ((reinterpret_cast<uintptr_t>(workspace) & 15u) || (reinterpret_cast<uintptr_t>(coef) & 15u)) return PF_ERR_ARG;
  ReconGeom g;
  recon_geom(header, orientation, &g);
  uint8_t* planes = static_cast<uint8_t*>(workspace);
  hipLaunchKernelGGL(jpeg_idct_kernel, dim3((g.nblocks + JT - 1) / JT), dim3(JT), 0, ST(stream), g, coef, planes);
  hipLaunchKernelGGL(jpeg_color_store_kernel, dim3((g.W + JT - 1) / JT, g.H), dim3(JT), 0, ST(stream), g, planes, rgb);
  return ok();
}
