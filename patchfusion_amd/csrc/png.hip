// PNG encoding of the two images the save path writes (estimator/tester/tester.py:66-76: cv2.imwrite of the colour image and
// PIL's 16-bit PNG of depth * 256), on the device arrays that colorize_bgr_kernel / depth_u16_kernel leave in HBM.
// A PNG row filter followed by Huffman coding of the filtered bytes as literals -- no LZ77 match search (zlib's Z_HUFFMAN_ONLY):
//   pass A  png_filter_hist_kernel  one wave per row: |residual as int8| sums of None / Sub / Up / Paeth, the smallest wins (libpng's
//                                   heuristic); the filter byte per row and one 257-bin histogram of the whole filtered stream
//                                   (filter bytes included, end-of-block = one per band), private in LDS, one flush per block.
//   host    pf_png_build_table      png_huff.h: canonical code <= 15 bits + the dynamic-block header, ~1 KB down and ~1.3 KB up.
//   pass B  png_encode_band_kernel  one workgroup per band of PF_PNG_BAND_ROWS rows = one non-final dynamic-Huffman block + an empty
//                                   stored block (sync flush), so every band starts on a byte boundary.  The residuals are RECOMPUTED
//                                   from the image and the row's filter byte (no filtered stream in HBM).  Four stream bytes per lane
//                                   are looked up and concatenated (<= 60 bits), a block prefix sum of the bit counts places them,
//                                   64-bit LDS atomic ORs merge them into a staging window that is flushed with 16-byte stores.
//                                   Per band: its byte count and its Adler-32 partial sums  S1 = sum b, S2 = sum (n - i) b  mod 65521.
//   pass C  png_scan_kernel + png_compact_kernel   exclusive scan of the band sizes, slots copied into one contiguous buffer.
// The stream byte (r, j) of pixel byte j is read through raw_at: 16-bit samples big-endian (torch.uint16 is little-endian), and the
// `bgr` flag swaps channels 0 and 2, so the array cv2.imwrite takes gives the file cv2 writes.
#include "png_dev.h"

namespace {

constexpr int PNG_HDR_BITS_MAX = pf_png::HDR_BYTES * 8;
constexpr int PNG_STAGE_WORDS = (PNG_HDR_BITS_MAX + PNG_CHUNK * 15) / 64 + 16;      // header + one chunk at 15 bits per byte + slack

// ------------------------------------------------------------------------------------------------ pass A
template <int BPP, int MODE>
__global__ __launch_bounds__(PNG_THREADS) void png_filter_hist_kernel(const uint8_t* __restrict__ img, int H, int rowbytes,
                                                                      uint8_t* __restrict__ filt, uint32_t* __restrict__ hist, int nbands) {
  __shared__ uint32_t h[pf_png::NSYM];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int i = tid; i < pf_png::NSYM; i += PNG_THREADS) h[i] = 0;
  __syncthreads();
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
    if (lane == 0) {
      filt[r] = (uint8_t)f;
      atomicAdd(&h[f], 1u);
    }
    for (int j = lane; j < rowbytes; j += 64) atomicAdd(&h[residual<BPP, MODE>(img, rb, rowbytes, (int)r, j, f)], 1u);
  }
  __syncthreads();
  for (int i = tid; i < pf_png::NSYM; i += PNG_THREADS)
    if (h[i]) atomicAdd(&hist[i], h[i]);
  if (blockIdx.x == 0 && tid == 0) atomicAdd(&hist[pf_png::EOB], (uint32_t)nbands);
}

// ------------------------------------------------------------------------------------------------ pass B
// meta: [0..1] total bytes (pass C), then per band {bytes, S1, S2}
template <int BPP, int MODE>
__global__ __launch_bounds__(PNG_THREADS) void png_encode_band_kernel(const uint8_t* __restrict__ img, int H, int rowbytes,
                                                                      const uint8_t* __restrict__ filt, const uint32_t* __restrict__ table,
                                                                      uint8_t* __restrict__ slots, long slot_bytes, uint32_t* __restrict__ meta) {
  __shared__ __attribute__((aligned(16))) unsigned long long stage[PNG_STAGE_WORDS];
  __shared__ uint32_t tab[pf_png::NSYM + 1];
  __shared__ uint32_t wt[PNG_WAVES];
  __shared__ uint32_t red[2 * PNG_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long band = blockIdx.x;
  const int r0 = (int)(band * PF_PNG_BAND_ROWS);
  const int rows = H - r0 < PF_PNG_BAND_ROWS ? H - r0 : PF_PNG_BAND_ROWS;
  const int S = rowbytes + 1;
  const int nb = rows * S;                                 // stream bytes of this band; symbol nb is the end-of-block
  const unsigned long long* __restrict__ hdr = reinterpret_cast<const unsigned long long*>(table + pf_png::HDR_WORD0);
  for (int i = tid; i <= pf_png::NSYM; i += PNG_THREADS) tab[i] = table[i];
  for (int w = tid; w < PNG_STAGE_WORDS; w += PNG_THREADS) stage[w] = w < pf_png::HDR_BYTES / 8 ? hdr[w] : 0ull;
  __syncthreads();
  uint32_t carry = tab[pf_png::NSYM] < (uint32_t)PNG_HDR_BITS_MAX ? tab[pf_png::NSYM] : (uint32_t)PNG_HDR_BITS_MAX;   // bits waiting in stage
  long written16 = 0;
  uint4* __restrict__ out16 = reinterpret_cast<uint4*>(slots + band * slot_bytes);
  uint32_t adl1 = 0, adl2 = 0;                             // this lane's share of S1 (plain, < 2^32) and S2 (mod 65521)

  for (int base = 0; base <= nb; base += PNG_CHUNK) {
    const int cend = base + PNG_CHUNK < nb ? base + PNG_CHUNK : nb;
    const int i0 = base + tid * PNG_E;
    unsigned long long v = 0;
    uint32_t len = 0, c1 = 0, c2 = 0;
    if (i0 <= nb) {
      int r = i0 / S, j = i0 - r * S;                      // j = 0 is the row's filter byte, j - 1 the pixel byte
      int f = r < rows ? filt[r0 + r] : 0;
#pragma unroll
      for (int e = 0; e < PNG_E; ++e) {
        const int i = i0 + e;
        if (i > nb) break;
        uint32_t sym;
        if (i == nb) {
          sym = pf_png::EOB;
        } else {
          sym = j == 0 ? (uint32_t)f : residual<BPP, MODE>(img, (long)(r0 + r) * rowbytes, rowbytes, r0 + r, j - 1, f);
          c1 += sym;
          c2 += (uint32_t)(cend - i) * sym;                // <= 4 * 1024 * 255
          if (++j == S) {
            j = 0;
            if (++r < rows) f = filt[r0 + r];
          }
        }
        const uint32_t t = tab[sym];
        v |= (unsigned long long)(t & 0xffffu) << len;
        len += (t >> 16) & 15u;
      }
    }
    adl1 += c1;
    adl2 = (adl2 + (uint32_t)((nb - cend) % (int)ADLER) * c1 + c2) % ADLER;       // 65520 * 1020 + 2^20 + 65520 < 2^32

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
    const uint32_t T = carry + total;                      // <= 2048 + 1024 * 15 bits
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

// ------------------------------------------------------------------------------------------------ pass C
__global__ __launch_bounds__(PNG_THREADS) void png_scan_kernel(uint32_t* __restrict__ meta, int nbands, unsigned long long* __restrict__ offsets) {
  __shared__ unsigned long long wt[PNG_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  unsigned long long carry = 0;
  for (int base = 0; base < nbands; base += PNG_THREADS) {
    const int i = base + tid;
    const unsigned long long v = i < nbands ? meta[2 + 3 * (long)i] : 0;
    unsigned long long incl = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const unsigned long long t = __shfl_up(incl, o, 64);
      if (lane >= o) incl += t;
    }
    if (lane == 63) wt[wave] = incl;
    __syncthreads();
    unsigned long long woff = 0, total = 0;
    for (int w = 0; w < PNG_WAVES; ++w) {
      if (w < wave) woff += wt[w];
      total += wt[w];
    }
    if (i < nbands) offsets[i] = carry + woff + incl - v;
    carry += total;
    __syncthreads();
  }
  if (tid == 0) {
    offsets[nbands] = carry;
    meta[0] = (uint32_t)carry;
    meta[1] = (uint32_t)(carry >> 32);
  }
}

// one block per band; the destination is written in aligned 16-byte units, each built from five aligned words of the slot
__global__ __launch_bounds__(PNG_THREADS) void png_compact_kernel(const uint8_t* __restrict__ slots, long slot_bytes, const uint32_t* __restrict__ meta,
                                                                  const unsigned long long* __restrict__ offsets, uint8_t* __restrict__ out) {
  const long band = blockIdx.x;
  const int tid = threadIdx.x;
  const long size = meta[2 + 3 * band];
  const uint8_t* __restrict__ src = slots + band * slot_bytes;
  uint8_t* __restrict__ dst = out + offsets[band];
  long head = (16 - (long)(reinterpret_cast<uintptr_t>(dst) & 15u)) & 15;
  if (head > size) head = size;
  for (long i = tid; i < head; i += PNG_THREADS) dst[i] = src[i];
  const long nbody = (size - head) >> 4;
  const uint32_t sh = (uint32_t)(head & 3) * 8u;
  const uint32_t* __restrict__ s32 = reinterpret_cast<const uint32_t*>(src) + (head >> 2);
  uint4* __restrict__ d16 = reinterpret_cast<uint4*>(dst + head);
  for (long u = tid; u < nbody; u += PNG_THREADS) {
    const uint32_t* p = s32 + 4 * u;
    uint4 d;
    if (sh == 0) {
      d = make_uint4(p[0], p[1], p[2], p[3]);
    } else {
      const uint32_t a0 = p[0], a1 = p[1], a2 = p[2], a3 = p[3], a4 = p[4];     // p[4] lies inside the slot: it ends with 16 spare bytes
      d = make_uint4((a0 >> sh) | (a1 << (32u - sh)), (a1 >> sh) | (a2 << (32u - sh)), (a2 >> sh) | (a3 << (32u - sh)),
                     (a3 >> sh) | (a4 << (32u - sh)));
    }
    d16[u] = d;
  }
  for (long i = head + 16 * nbody + tid; i < size; i += PNG_THREADS) dst[i] = src[i];
}

// ------------------------------------------------------------------------------------------------ host
template <int BPP, int MODE>
void launch_a(const void* img, int H, const Geom& g, uint8_t* filt, uint32_t* hist, hipStream_t s) {
  int grid = (H + PNG_WAVES - 1) / PNG_WAVES;
  if (grid > 2048) grid = 2048;
  hipLaunchKernelGGL((png_filter_hist_kernel<BPP, MODE>), dim3(grid), dim3(PNG_THREADS), 0, s, static_cast<const uint8_t*>(img), H,
                     (int)g.rowbytes, filt, hist, g.nbands);
}
template <int BPP, int MODE>
void launch_b(const void* img, int H, const Geom& g, const uint8_t* filt, const uint32_t* table, uint8_t* slots, uint32_t* meta, hipStream_t s) {
  hipLaunchKernelGGL((png_encode_band_kernel<BPP, MODE>), dim3(g.nbands), dim3(PNG_THREADS), 0, s, static_cast<const uint8_t*>(img), H,
                     (int)g.rowbytes, filt, table, slots, g.slot_bytes, meta);
}

}  // namespace

int pf_png::launch_scan_compact(uint32_t* meta, int nbands, unsigned long long* offsets, const uint8_t* slots, long slot_bytes, uint8_t* out,
                                hipStream_t stream) {
  hipLaunchKernelGGL(png_scan_kernel, dim3(1), dim3(PNG_THREADS), 0, stream, meta, nbands, offsets);
  hipLaunchKernelGGL(png_compact_kernel, dim3(nbands), dim3(PNG_THREADS), 0, stream, slots, slot_bytes, meta, offsets, out);
  return ok();
}

extern "C" int pf_png_workspace_bytes(int H, int W, int channels, int bits, long* workspace_bytes, long* out_bytes, int* nbands) {
  Geom g;
  if (!workspace_bytes || !out_bytes || !nbands || !png_geom(H, W, channels, bits, 0, &g)) return PF_ERR_ARG;
  *workspace_bytes = g.filt_bytes + g.off_bytes + (long)g.nbands * g.slot_bytes;
  *out_bytes = (long)g.nbands * g.slot_bytes;
  *nbands = g.nbands;
  return PF_OK;
}

extern "C" int pf_png_filter_histogram(const void* img, int H, int W, int channels, int bits, int bgr, void* workspace, uint32_t* hist257,
                                       void* stream) {
  Geom g;
  if (!img || !workspace || !hist257 || !png_geom(H, W, channels, bits, bgr, &g)) return PF_ERR_ARG;
  if ((reinterpret_cast<uintptr_t>(workspace) & 15u) || (reinterpret_cast<uintptr_t>(hist257) & 3u)) return PF_ERR_ARG;
  if (hipMemsetAsync(hist257, 0, pf_png::NSYM * sizeof(uint32_t), ST(stream)) != hipSuccess) return PF_ERR_LAUNCH;
  uint8_t* filt = static_cast<uint8_t*>(workspace);
  PNG_DISPATCH(launch_a, img, H, g, filt, hist257, ST(stream));
  return ok();
}

extern "C" int pf_png_build_table(const uint32_t* hist257, uint32_t* table) {
  return pf_png::build_table(hist257, table) ? PF_ERR_ARG : PF_OK;
}

extern "C" int pf_png_encode(const void* img, int H, int W, int channels, int bits, int bgr, const uint32_t* table, void* workspace,
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
  return pf_png::launch_scan_compact(meta, g.nbands, offsets, slots, g.slot_bytes, out, ST(stream));
}
