// Run matches for the device PNG encoder (estimator/tester/tester.py:66-76, the files csrc/png.hip writes with literals only): the
// same row filters, bands, slots and pass C, with every stretch of equal bytes inside a stream row coded as deflate matches at
// distance 1 (zlib's Z_RLE).  No hash chains and no search window: a run is found from "equals its predecessor" flags alone.
//
// Token rule, shared by both passes and by the numpy model in tests/png_rle_ref.py.  A row of the filtered stream is its filter byte
// and rowbytes residuals, S bytes.  A run is a maximal stretch of equal bytes inside one row; position p = 0 .. L-1 inside it:
//   p = 0            the literal v
//   p = 1 + 258 c    first byte of a chunk of m = min(258, L - p) bytes: m >= 3 -> one match (length symbol 257 .. 285, its extra
//                    bits, the one-bit distance code of distance 1); m < 3 -> a literal here and, for m = 2, at the next byte
//   everything else  nothing
// Runs never cross rows, so they never cross bands, and a band stays one self-contained deflate block.
//
//   pass A'  png_rle_filter_hist_kernel  one wave per row, the filter choice of png_filter_hist_kernel; the second sweep counts the
//                                        257-bin literal histogram AND, run by run, the 286-bin token histogram and the total of
//                                        extra bits.  A run is closed by the lane that holds the head of the next one: its head is
//                                        the highest head flag below that lane in the wave's ballot, or the one carried from
//                                        earlier strides of the row.
//   host     pf_png_rle_build_table      png_huff.h: code <= 14 bits over 286 symbols + header, 388 words.
//   pass B'  png_rle_encode_band_kernel  one workgroup per band.  Chunks of 1024 stream bytes are taken one ahead: the residuals
//                                        of chunk c + 1 are computed (once) and their head flags published as a bit mask in LDS
//                                        before chunk c is coded, so that a match start finds its run's end, at most 258 bytes
//                                        ahead, with a find-first-set over at most five 64-bit words.  The way back to the run's
//                                        head has no bound (a constant row is one run): an inclusive max-scan of head positions
//                                        over the workgroup, carried from chunk to chunk.  Bit placement, staging window, sync
//                                        flush and Adler-32 partial sums are those of png_encode_band_kernel.
//   pass C   pf_png::launch_scan_compact (png.hip), unchanged.
#include "png_dev.h"

namespace {

using pf_png::EOB;

constexpr int RLE_HDR_BITS_MAX = pf_png::RLE_HDR_BYTES * 8;
// header + one chunk: four stream bytes of a lane give <= 62 bits (three literals and a match), + slack as in png.hip
constexpr int RLE_STAGE_WORDS = (RLE_HDR_BITS_MAX + PNG_THREADS * 62) / 64 + 16;
constexpr int RLE_HIST_LIT = 0, RLE_HIST_TOK = 257, RLE_HIST_EXTRA = 544;           // word offsets in the PF_PNG_RLE_HIST_WORDS buffer
constexpr int MAX_MATCH = 258;

// match length 3 .. 258 -> length symbol, number of extra bits (the extra value is (len - 3) & ((1 << bits) - 1)); RFC 1951 3.2.5
__device__ __forceinline__ void length_symbol(uint32_t len, uint32_t* sym, uint32_t* ebits) {
  const uint32_t l = len - 3u;
  if (l < 8u) { *sym = 257u + l; *ebits = 0; return; }
  if (len == (uint32_t)MAX_MATCH) { *sym = 285u; *ebits = 0; return; }
  const uint32_t e = 29u - (uint32_t)__clz(l);             // 31 - clz = index of the top bit (>= 3), two bits below it select the symbol
  *sym = 261u + 4u * e + ((l >> e) & 3u);
  *ebits = e;
}

// ------------------------------------------------------------------------------------------------ pass A'
// hist: [0 .. 256] literal histogram as png_filter_hist_kernel writes it, [257 .. 542] token histogram, [544 .. 545] extra bits (64-bit)
template <int BPP, int MODE>
__global__ __launch_bounds__(PNG_THREADS) void png_rle_filter_hist_kernel(const uint8_t* __restrict__ img, int H, int rowbytes,
                                                                          uint8_t* __restrict__ filt, uint32_t* __restrict__ hist, int nbands) {
  __shared__ uint32_t h[pf_png::NSYM];
  __shared__ uint32_t t[pf_png::RLE_NSYM];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int i = tid; i < pf_png::NSYM; i += PNG_THREADS) h[i] = 0;
  for (int i = tid; i < pf_png::RLE_NSYM; i += PNG_THREADS) t[i] = 0;
  __syncthreads();
  const int S = rowbytes + 1;
  unsigned long long extra = 0;
  for (long r = (long)blockIdx.x * PNG_WAVES + wave; r < H; r += (long)gridDim.x * PNG_WAVES) {
    const long rb = r * rowbytes;
    unsigned long long s0 = 0, s1 = 0, s2 = 0, s4 = 0;
    for (int j = lane; j < rowbytes; j += 64) {
      const uint32_t x = raw_at<BPP, MODE>(img, rb, j);
      const uint32_t a = j >= BPP ? raw_at<BPP, MODE>(img, rb, j - BPP) : 0u;
      const uint32_t b = r > 0 ? raw_at<BPP, MODE>(img, rb - rowbytes, j) : 0u;
      const uint32_t c = (r > 0 && j >= BPP) ? raw_at<BPP, MODE>(img, rb - rowbytes, j - BPP) : 0u;
      s0 += abs_i8(x);
      s1 += abs_i8(x - a);
      s2 += abs_i8(x - b);
      s4 += abs_i8(x - paeth((int)a, (int)b, (int)c));
    }
    s0 = wave_sum_u64(s0); s1 = wave_sum_u64(s1); s2 = wave_sum_u64(s2); s4 = wave_sum_u64(s4);
    int f = 0;                                             // ties go to the earlier of None, Sub, Up, Paeth
    unsigned long long best = s0;
    if (s1 < best) { best = s1; f = 1; }
    if (s2 < best) { best = s2; f = 2; }
    if (s4 < best) { best = s4; f = 4; }
    if (lane == 0) filt[r] = (uint8_t)f;

    // stream positions 0 .. S-1 in strides of 64, and position S as the head that closes the last run
    uint32_t last = 0;                                     // the byte before this stride
    int carry_head = 0;                                    // head of the run that is open at the start of this stride
    for (int j0 = 0; j0 <= S; j0 += 64) {
      const int j = j0 + lane;
      uint32_t v = 0;
      if (j < S) {
        v = j == 0 ? (uint32_t)f : residual<BPP, MODE>(img, rb, rowbytes, (int)r, j - 1, f);
        atomicAdd(&h[v], 1u);
      }
      uint32_t pv = __shfl_up(v, 1, 64);
      if (lane == 0) pv = last;
      const bool head = j <= S && (j == 0 || j == S || v != pv);
      const unsigned long long heads = __ballot(head);
      if (head && j > 0) {                                 // closes the run of pv that ends at j - 1
        const unsigned long long below = heads & ((1ull << lane) - 1ull);
        const int hd = below ? j0 + 63 - __clzll((long long)below) : carry_head;
        const uint32_t rest = (uint32_t)(j - hd - 1);      // bytes after the literal at the head
        const uint32_t full = rest / (uint32_t)MAX_MATCH, tail = rest % (uint32_t)MAX_MATCH;
        atomicAdd(&t[pv], 1u + (tail < 3u ? tail : 0u));
        if (full) atomicAdd(&t[285], full);
        if (tail >= 3u) {
          uint32_t sym, eb;
          length_symbol(tail, &sym, &eb);
          atomicAdd(&t[sym], 1u);
          extra += eb;
        }
      }
      if (heads) carry_head = j0 + 63 - __clzll((long long)heads);
      last = __shfl(v, 63, 64);
    }
  }
  extra = wave_sum_u64(extra);
  __syncthreads();
  for (int i = tid; i < pf_png::NSYM; i += PNG_THREADS)
    if (h[i]) atomicAdd(&hist[RLE_HIST_LIT + i], h[i]);
  for (int i = tid; i < pf_png::RLE_NSYM; i += PNG_THREADS)
    if (t[i]) atomicAdd(&hist[RLE_HIST_TOK + i], t[i]);
  if (lane == 0 && extra) atomicAdd(reinterpret_cast<unsigned long long*>(hist + RLE_HIST_EXTRA), extra);
  if (blockIdx.x == 0 && tid == 0) {
    atomicAdd(&hist[RLE_HIST_LIT + EOB], (uint32_t)nbands);
    atomicAdd(&hist[RLE_HIST_TOK + EOB], (uint32_t)nbands);
  }
}

// ------------------------------------------------------------------------------------------------ pass B'
// min(258, distance from position `pos` of the 2048-bit head-flag ring to the next head after it)
__device__ __forceinline__ uint32_t run_ahead(const unsigned long long* heads, uint32_t pos) {
  const uint32_t s = pos + 1u;
  uint32_t w = (s >> 6) & 31u;
  unsigned long long m = heads[w] >> (s & 63u);
  if (m) return 1u + (uint32_t)__builtin_ctzll(m);
  uint32_t d = 65u - (s & 63u);                            // distance to bit 0 of the next word
#pragma unroll 1
  for (int k = 0; k < 4 && d < (uint32_t)MAX_MATCH; ++k, d += 64u) {
    w = (w + 1u) & 31u;
    m = heads[w];
    if (m) {
      d += (uint32_t)__builtin_ctzll(m);
      return d < (uint32_t)MAX_MATCH ? d : (uint32_t)MAX_MATCH;
    }
  }
  return (uint32_t)MAX_MATCH;
}

// meta: [0..1] total bytes (pass C), then per band {bytes, S1, S2}
template <int BPP, int MODE>
__global__ __launch_bounds__(PNG_THREADS) void png_rle_encode_band_kernel(const uint8_t* __restrict__ img, int H, int rowbytes,
                                                                          const uint8_t* __restrict__ filt, const uint32_t* __restrict__ table,
                                                                          uint8_t* __restrict__ slots, long slot_bytes,
                                                                          uint32_t* __restrict__ meta) {
  __shared__ __attribute__((aligned(16))) unsigned long long stage[RLE_STAGE_WORDS];
  __shared__ unsigned long long heads[32];                 // head flags of two chunks, one bit per stream byte, chunk c in words 16 (c & 1) ..
  __shared__ uint32_t tab[pf_png::RLE_DIST_WORD + 1];
  __shared__ uint32_t wt[PNG_WAVES];
  __shared__ int whead[2][PNG_WAVES];
  __shared__ uint32_t red[2 * PNG_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long band = blockIdx.x;
  const int r0 = (int)(band * PF_PNG_BAND_ROWS);
  const int rows = H - r0 < PF_PNG_BAND_ROWS ? H - r0 : PF_PNG_BAND_ROWS;
  const int S = rowbytes + 1;
  const int nb = rows * S;                                 // stream bytes of this band; symbol nb is the end-of-block
  const unsigned long long* __restrict__ hdr = reinterpret_cast<const unsigned long long*>(table + pf_png::RLE_HDR_WORD0);
  for (int i = tid; i <= pf_png::RLE_DIST_WORD; i += PNG_THREADS) tab[i] = table[i];
  for (int w = tid; w < RLE_STAGE_WORDS; w += PNG_THREADS) stage[w] = w < pf_png::RLE_HDR_BYTES / 8 ? hdr[w] : 0ull;
  uint32_t carry = table[pf_png::RLE_HDR_BITS_WORD] < (uint32_t)RLE_HDR_BITS_MAX ? table[pf_png::RLE_HDR_BITS_WORD]
                                                                                 : (uint32_t)RLE_HDR_BITS_MAX;   // bits waiting in stage
  long written16 = 0;
  uint4* __restrict__ out16 = reinterpret_cast<uint4*>(slots + band * slot_bytes);
  uint32_t adl1 = 0, adl2 = 0;                             // this lane's share of S1 (plain, < 2^32) and S2 (mod 65521)
  int carry_head = 0;                                      // the last head before the chunk being loaded (position 0 is always one)

  // Chunk `base`: this lane's four stream bytes (packed, byte e = position base + 4 tid + e), their head flags (bit e: first byte of a
  // run; a row start, the end-of-block and everything behind it are heads), and the head of the run open just before the lane's bytes.
  // Publishes the flags in heads; the caller synchronises before it reads them.  Also folds the chunk into the Adler-32 sums.
  uint32_t bytes = 0, flags = 0;
  int head_before = 0;
  auto load_chunk = [&](int base, uint32_t* bytes_out, uint32_t* flags_out, int* lane_scan) {
    const int cend = base + PNG_CHUNK < nb ? base + PNG_CHUNK : nb;
    const int i0 = base + tid * PNG_E;
    uint32_t pk = 0, fl = 0, c1 = 0, c2 = 0;
    int own = -1;                                          // the last head among this lane's bytes
    if (i0 < nb) {
      int r = i0 / S, j = i0 - r * S;                      // j = 0 is the row's filter byte, j - 1 the pixel byte
      int f = filt[r0 + r];
      uint32_t prev = j >= 2 ? residual<BPP, MODE>(img, (long)(r0 + r) * rowbytes, rowbytes, r0 + r, j - 2, f) : (uint32_t)f;
#pragma unroll
      for (int e = 0; e < PNG_E; ++e) {
        const int i = i0 + e;
        if (i >= nb) { fl |= 1u << e; own = i; continue; }
        const uint32_t sym = j == 0 ? (uint32_t)f : residual<BPP, MODE>(img, (long)(r0 + r) * rowbytes, rowbytes, r0 + r, j - 1, f);
        c1 += sym;
        c2 += (uint32_t)(cend - i) * sym;                  // <= 4 * 1024 * 255
        pk |= sym << (8 * e);
        if (j == 0 || sym != prev) { fl |= 1u << e; own = i; }
        prev = sym;
        if (++j == S) {
          j = 0;
          if (++r < rows) f = filt[r0 + r];
        }
      }
    } else {
      fl = 15u;
      own = i0 + PNG_E - 1;
    }
    adl1 += c1;
    adl2 = (adl2 + (uint32_t)((nb - cend) % (int)ADLER) * c1 + c2) % ADLER;       // 65520 * 1020 + 2^20 + 65520 < 2^32
    // sixteen lanes share a 64-bit word of flags
    unsigned long long word = (unsigned long long)fl << (4 * (lane & 15));
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) word |= __shfl_xor(word, o, 64);
    if ((lane & 15) == 0) heads[((base / PNG_CHUNK) & 1) * 16 + (tid >> 4)] = word;
    int incl = own;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int t = __shfl_up(incl, o, 64);
      if (lane >= o && t > incl) incl = t;
    }
    if (lane == 63) whead[(base / PNG_CHUNK) & 1][wave] = incl;
    int before = __shfl_up(incl, 1, 64);
    if (lane == 0) before = -1;
    *bytes_out = pk;
    *flags_out = fl;
    *lane_scan = before;
  };
  // after the synchronisation: the head before this lane's bytes, and the carry for the next chunk
  auto finish_chunk = [&](int base, int lane_scan) {
    const int* wh = whead[(base / PNG_CHUNK) & 1];
    int before = lane_scan > carry_head ? lane_scan : carry_head;
#pragma unroll
    for (int w = 0; w < PNG_WAVES; ++w) {
      if (w < wave && wh[w] > before) before = wh[w];
      if (wh[w] > carry_head) carry_head = wh[w];
    }
    return before;
  };

  {
    int scan;
    load_chunk(0, &bytes, &flags, &scan);
    __syncthreads();
    head_before = finish_chunk(0, scan);
  }

  for (int base = 0; base <= nb; base += PNG_CHUNK) {
    uint32_t nbytes, nflags;
    int nscan;
    load_chunk(base + PNG_CHUNK, &nbytes, &nflags, &nscan);
    __syncthreads();
    const int nhead_before = finish_chunk(base + PNG_CHUNK, nscan);

    const int i0 = base + tid * PNG_E;
    const uint32_t ring0 = (uint32_t)(((base / PNG_CHUNK) & 1) * PNG_CHUNK + tid * PNG_E);
    unsigned long long v = 0;
    uint32_t len = 0;
    int head = head_before;
#pragma unroll
    for (int e = 0; e < PNG_E; ++e) {
      const int i = i0 + e;
      if (i > nb) break;
      if ((flags >> e) & 1u) head = i;
      const uint32_t p = (uint32_t)(i - head);
      uint32_t lit = i == nb ? (uint32_t)EOB : ((bytes >> (8 * e)) & 255u);
      bool emit = true;
      if (p) {
        const uint32_t q = (p - 1u) % (uint32_t)MAX_MATCH;
        if (q == 0) {
          const uint32_t m = run_ahead(heads, ring0 + e);
          if (m >= 3u) {
            uint32_t sym, eb;
            length_symbol(m, &sym, &eb);
            const uint32_t t = tab[sym], d = tab[pf_png::RLE_DIST_WORD];
            v |= (unsigned long long)(t & 0xffffu) << len;
            len += (t >> 16) & 15u;
            v |= (unsigned long long)((m - 3u) & ((1u << eb) - 1u)) << len;
            len += eb;
            v |= (unsigned long long)(d & 0xffffu) << len;
            len += (d >> 16) & 15u;
            emit = false;
          }
        } else {
          // second byte of a chunk: a literal only where the chunk is two bytes long, i.e. the next position is a head
          emit = q == 1u && ((heads[((ring0 + e + 1u) >> 6) & 31u] >> ((ring0 + e + 1u) & 63u)) & 1ull);
        }
      }
      if (emit) {
        const uint32_t t = tab[lit];
        v |= (unsigned long long)(t & 0xffffu) << len;
        len += (t >> 16) & 15u;
      }
    }

    uint32_t incl = len;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t t = __shfl_up(incl, o, 64);
      if (lane >= o) incl += t;
    }
    if (lane == 63) wt[wave] = incl;
    __syncthreads();
    uint32_t woff = 0, total = 0;
#pragma unroll
    for (int w = 0; w < PNG_WAVES; ++w) {
      if (w < wave) woff += wt[w];
      total += wt[w];
    }
    if (len) {
      const uint32_t off = carry + woff + incl - len;
      const uint32_t w = off >> 6, sh = off & 63u;
      atomicOr(&stage[w], v << sh);
      if (sh + len > 64u) atomicOr(&stage[w + 1], v >> (64u - sh));
    }
    __syncthreads();
    const uint32_t T = carry + total;                      // <= 2176 + 256 * 62 bits
    const uint32_t n16 = T >> 7;
    const uint4* st16 = reinterpret_cast<const uint4*>(stage);
    for (uint32_t u = tid; u < n16; u += PNG_THREADS) out16[written16 + u] = st16[u];
    const unsigned long long keep0 = stage[2 * n16], keep1 = stage[2 * n16 + 1];
    __syncthreads();
    const uint32_t nw = ((T + 63u) >> 6) + 1u;
    for (uint32_t w = tid; w < nw; w += PNG_THREADS) stage[w] = w == 0 ? keep0 : (w == 1 ? keep1 : 0ull);
    __syncthreads();
    carry = T & 127u;
    written16 += n16;
    bytes = nbytes;
    flags = nflags;
    head_before = nhead_before;
  }

  // sync flush: an empty stored block (BFINAL = 0, BTYPE = 0, pad to a byte, LEN = 0, NLEN = 0xffff)
  carry = (carry + 3u + 7u) & ~7u;
  if (tid == 0) {
    const uint32_t w = carry >> 6, sh = carry & 63u;
    stage[w] |= 0xffff0000ull << sh;
    if (sh + 32u > 64u) stage[w + 1] |= 0xffff0000ull >> (64u - sh);
  }
  carry += 32u;
  __syncthreads();
  const uint32_t n16 = (carry + 127u) >> 7;                // <= 2; the slot is a multiple of 16 bytes
  const uint4* st16 = reinterpret_cast<const uint4*>(stage);
  if ((uint32_t)tid < n16) out16[written16 + tid] = st16[tid];

  adl1 %= ADLER;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    adl1 += __shfl_xor(adl1, o, 64);
    adl2 += __shfl_xor(adl2, o, 64);
  }
  if (lane == 0) { red[wave] = adl1; red[PNG_WAVES + wave] = adl2; }
  __syncthreads();
  if (tid == 0) {
    uint32_t a = 0, b = 0;
    for (int w = 0; w < PNG_WAVES; ++w) { a += red[w]; b += red[PNG_WAVES + w]; }
    uint32_t* m = meta + 2 + 3 * band;
    m[0] = (uint32_t)(written16 * 16 + (carry >> 3));
    m[1] = a % ADLER;
    m[2] = b % ADLER;
  }
}

// ------------------------------------------------------------------------------------------------ host
template <int BPP, int MODE>
void launch_a(const void* img, int H, const Geom& g, uint8_t* filt, uint32_t* hist, hipStream_t s) {
  int grid = (H + PNG_WAVES - 1) / PNG_WAVES;
  if (grid > 2048) grid = 2048;
  hipLaunchKernelGGL((png_rle_filter_hist_kernel<BPP, MODE>), dim3(grid), dim3(PNG_THREADS), 0, s, static_cast<const uint8_t*>(img), H,
                     (int)g.rowbytes, filt, hist, g.nbands);
}
template <int BPP, int MODE>
void launch_b(const void* img, int H, const Geom& g, const uint8_t* filt, const uint32_t* table, uint8_t* slots, uint32_t* meta, hipStream_t s) {
  hipLaunchKernelGGL((png_rle_encode_band_kernel<BPP, MODE>), dim3(g.nbands), dim3(PNG_THREADS), 0, s, static_cast<const uint8_t*>(img), H,
                     (int)g.rowbytes, filt, table, slots, g.rle_slot_bytes, meta);
}

inline long max_slot(const Geom& g) { return g.slot_bytes > g.rle_slot_bytes ? g.slot_bytes : g.rle_slot_bytes; }

}  // namespace

extern "C" int pf_png_rle_workspace_bytes(int H, int W, int channels, int bits, long* workspace_bytes, long* out_bytes, int* nbands) {
  Geom g;
  if (!workspace_bytes || !out_bytes || !nbands || !png_geom(H, W, channels, bits, 0, &g)) return PF_ERR_ARG;
  *workspace_bytes = g.filt_bytes + g.off_bytes + (long)g.nbands * max_slot(g);
  *out_bytes = (long)g.nbands * max_slot(g);
  *nbands = g.nbands;
  return PF_OK;
}

extern "C" int pf_png_rle_filter_histogram(const void* img, int H, int W, int channels, int bits, int bgr, void* workspace, uint32_t* hist,
                                           void* stream) {
  Geom g;
  if (!img || !workspace || !hist || !png_geom(H, W, channels, bits, bgr, &g)) return PF_ERR_ARG;
  if ((reinterpret_cast<uintptr_t>(workspace) & 15u) || (reinterpret_cast<uintptr_t>(hist) & 7u)) return PF_ERR_ARG;
  if (hipMemsetAsync(hist, 0, PF_PNG_RLE_HIST_WORDS * sizeof(uint32_t), ST(stream)) != hipSuccess) return PF_ERR_LAUNCH;
  uint8_t* filt = static_cast<uint8_t*>(workspace);
  PNG_DISPATCH(launch_a, img, H, g, filt, hist, ST(stream));
  return ok();
}

extern "C" int pf_png_rle_build_table(const uint32_t* hist286, uint32_t* table) {
  return pf_png::build_rle_table(hist286, table) ? PF_ERR_ARG : PF_OK;
}

extern "C" int pf_png_rle_encode(const void* img, int H, int W, int channels, int bits, int bgr, const uint32_t* table, void* workspace,
                                 uint8_t* out, uint32_t* meta, void* stream) {
  Geom g;
  if (!img || !table || !workspace || !out || !meta || !png_geom(H, W, channels, bits, bgr, &g)) return PF_ERR_ARG;
  if ((reinterpret_cast<uintptr_t>(workspace) & 15u) || (reinterpret_cast<uintptr_t>(table) & 7u) || (reinterpret_cast<uintptr_t>(meta) & 3u))
    return PF_ERR_ARG;
  uint8_t* ws = static_cast<uint8_t*>(workspace);
  const uint8_t* filt = ws;
  unsigned long long* offsets = reinterpret_cast<unsigned long long*>(ws + g.filt_bytes);
  uint8_t* slots = ws + g.filt_bytes + g.off_bytes;
  PNG_DISPATCH(launch_b, img, H, g, filt, table, slots, meta, ST(stream));
  return pf_png::launch_scan_compact(meta, g.nbands, offsets, slots, g.rle_slot_bytes, out, ST(stream));
}
