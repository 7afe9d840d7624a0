// What the two translation units of the device PNG encoder share: png.hip (every filtered byte a literal) and png_rle.hip (run matches at
// distance 1).  The byte layouts, the row filters, the band geometry with both slot bounds, and the launcher of pass C, which lives in
// png.hip and serves both encoders unchanged.
#pragma once
#include "pf_common.h"
#include "../../include/pf_hip.h"
#include "png_huff.h"

namespace pf_png {
// pass C (png.hip): exclusive scan of the band sizes in meta, then the slots copied back to back into out; returns a PF_* status
int launch_scan_compact(uint32_t* meta, int nbands, unsigned long long* offsets, const uint8_t* slots, long slot_bytes, uint8_t* out,
                        hipStream_t stream);
}  // namespace pf_png

namespace {

inline int ok() { return hipGetLastError() == hipSuccess ? PF_OK : PF_ERR_LAUNCH; }
#define ST(s) reinterpret_cast<hipStream_t>(s)

constexpr int PNG_THREADS = 256, PNG_WAVES = PNG_THREADS / 64;
constexpr int PNG_E = 4;                                  // stream bytes per lane and chunk: 4 codes <= 60 bits in one 64-bit word
constexpr int PNG_CHUNK = PNG_THREADS * PNG_E;
constexpr uint32_t ADLER = 65521u;

// MODE 0: bytes as stored; 1: channels 0 and 2 swapped (BPP 3 / 4); 2: the two bytes of a 16-bit sample swapped (BPP 2)
template <int BPP, int MODE> __device__ __forceinline__ uint32_t raw_at(const uint8_t* __restrict__ img, long rowbase, int j) {
  int k = j;
  if (MODE == 1) {
    const int c = j % BPP;
    k = j - c + (c == 0 ? 2 : (c == 2 ? 0 : c));
  }
  if (MODE == 2) k = j ^ 1;
  return img[rowbase + k];
}

__device__ __forceinline__ uint32_t paeth(int a, int b, int c) {
  const int p = a + b - c;
  const int pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
  return (uint32_t)((pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c));
}

// filtered byte of row r (rowbase = r * rowbytes), byte j, filter f; row -1 and the bytes left of the first pixel are zeros
template <int BPP, int MODE>
__device__ __forceinline__ uint32_t residual(const uint8_t* __restrict__ img, long rowbase, int rowbytes, int r, int j, int f) {
  const uint32_t x = raw_at<BPP, MODE>(img, rowbase, j);
  if (f == 0) return x;
  const uint32_t a = j >= BPP ? raw_at<BPP, MODE>(img, rowbase, j - BPP) : 0u;
  if (f == 1) return (x - a) & 255u;
  const uint32_t b = r > 0 ? raw_at<BPP, MODE>(img, rowbase - rowbytes, j) : 0u;
  if (f == 2) return (x - b) & 255u;
  const uint32_t c = (r > 0 && j >= BPP) ? raw_at<BPP, MODE>(img, rowbase - rowbytes, j - BPP) : 0u;
  return (x - paeth((int)a, (int)b, (int)c)) & 255u;
}

__device__ __forceinline__ uint32_t abs_i8(uint32_t v) { v &= 255u; return v < 128u ? v : 256u - v; }

__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

struct Geom {
  int bpp, mode, nbands;
  long rowbytes, slot_bytes, rle_slot_bytes, filt_bytes, off_bytes;
};

inline long up16(long v) { return (v + 15) & ~15L; }

// channels 1 / 3 / 4 at 8 bits, channel 1 at 16 bits; bgr needs three channels
inline bool png_geom(int H, int W, int channels, int bits, int bgr, Geom* g) {
  if (H <= 0 || W <= 0) return false;
  if (bits == 8 && (channels == 1 || channels == 3 || channels == 4)) g->bpp = channels;
  else if (bits == 16 && channels == 1) g->bpp = 2;
  else return false;
  if (bgr && channels < 3) return false;
  g->mode = bits == 16 ? 2 : (bgr ? 1 : 0);
  g->rowbytes = (long)W * g->bpp;
  if ((g->rowbytes + 1) * PF_PNG_BAND_ROWS > 0x7fff0000L) return false;          // 32-bit stream index inside a band
  g->nbands = (H + PF_PNG_BAND_ROWS - 1) / PF_PNG_BAND_ROWS;
  // header + 15 bits per stream byte and for the end-of-block + stored block (3 + 7 + 32 bits), rounded to the 16-byte stores, + 16 spare
  g->slot_bytes = up16(pf_png::HDR_BYTES + (((g->rowbytes + 1) * PF_PNG_BAND_ROWS + 1) * 15 + 7) / 8 + 8) + 16;
  // run-match coding: a literal is <= 14 bits and a match (<= 14 + 5 + 1 bits) stands for >= 3 stream bytes: 14 bits per byte bound both
  g->rle_slot_bytes = up16(pf_png::RLE_HDR_BYTES + (((g->rowbytes + 1) * PF_PNG_BAND_ROWS + 1) * pf_png::RLE_MAX_BITS + 7) / 8 + 8) + 16;
  g->filt_bytes = up16(H);
  g->off_bytes = up16(((long)g->nbands + 1) * 8);
  return true;
}

#define PNG_DISPATCH(fn, ...)                                        \
  switch (g.bpp * 4 + g.mode) {                                      \
    case 1 * 4 + 0: fn<1, 0>(__VA_ARGS__); break;                    \
    case 2 * 4 + 2: fn<2, 2>(__VA_ARGS__); break;                    \
    case 3 * 4 + 0: fn<3, 0>(__VA_ARGS__); break;                    \
    case 3 * 4 + 1: fn<3, 1>(__VA_ARGS__); break;                    \
    case 4 * 4 + 0: fn<4, 0>(__VA_ARGS__); break;                    \
    default: fn<4, 1>(__VA_ARGS__); break;                           \
  }

}  // namespace
