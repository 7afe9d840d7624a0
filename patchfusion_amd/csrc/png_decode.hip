// PNG decoding on the device (include/pf_hip.h, "PNG decoding"): the deflate stream of a non-interlaced file is inflated block-parallel,
// then unfiltered and expanded.  Parsing and the chain walk are host code (png_host.h, preprocess.decode_png); the deflate code itself is
// png_inflate.h, shared with the host.
//
// A deflate block is an independent Huffman stream once its first bit is known.  The finder tests every bit offset for a well-formed
// dynamic header (a rare pattern); the scan pass decodes every candidate to its end-of-block code without storing, which gives the host
// the end bit and the output size of each; the host walks the chain of true blocks from bit 0 and sums their sizes; the inflate pass
// decodes each true block again, storing literals and, per output byte, the place it is copied from: its own place for a literal,
// otherwise the root of its match source, which after this pass is a literal's place or a place in a strictly earlier block.  Pointer
// jumping then resolves the places that still point into an earlier block (a chain visits a block at most once, so ceil(log2(blocks))
// rounds suffice; one more is run), and one gather makes the bytes.  A false candidate costs a wasted wave and nothing else: the walk
// never reaches it.
//
// Unfilter: a wave owns one dependent run of rows (a row with filter 0 or 1 needs nothing from the row above and starts a run) and works
// through it in bands of NR rows, one row per lane, skewed by one pixel: lane l handles pixel t - l at step t, so the pixel above (b) and
// above-left (c) were finished by lane l - 1 one and two steps earlier.  A band moves through a two-tile ring in LDS (64 pixels per tile
// and row, loaded and stored coalesced); the row above the band sits in ring row 0.
//
// The scan and inflate passes give a block to one wave.  Lane 0 builds the block's tables in LDS (canonical counts and symbols plus a
// 10-bit and an 8-bit lookup); then all 64 lanes decode the same symbols in step, which costs nothing on a SIMD and lets a match be
// copied by the whole wave.  Decoding inside a block is sequential: one symbol after the other.
//
// Termination and bounds (the invariants every kernel below keeps):
//   * no kernel waits on a word another workgroup of the same launch writes: every dependency is a kernel boundary on the one stream
//     (the in-place pointer jump reads words other threads may be replacing, but either value is an ancestor on the same chain and it
//     never waits for one);
//   * every loop over file data has a bound that is not data: the symbol loop runs while p < stop <= nbits and consumes at least one bit
//     per turn; header loops are bounded by 19 and 316; a match by 258; the run search by the height; the jump rounds are a fixed count;
//   * every bit read goes through peek(): 0 at or past nbits, otherwise words p / 32 .. p / 32 + PF_PNGD_PAD_WORDS - 1 of the
//     zero-padded buffer ((nbits + 31) / 32 + PF_PNGD_PAD_WORDS words, which the entry points are told and check);
//   * the scan pass stores only its own record; the finder stores list[i] only for i < capacity;
//   * the inflate pass stores lit[o] and ref[o] only for o inside its block's [offset, offset + bytes), which it first checks against the
//     expected inflated size; a match source is checked against the start of the output; ref[o] <= o always, so the jump and gather
//     kernels index inside [0, n);
//   * a stored block's source range is checked against the stream;
//   * unfilter and expand index rows < height and bytes < rowbytes only; a filter type above 4 and a palette index past PLTE set a flag
//     and decode as 0.
#include "pf_common.h"
#include "../../include/pf_hip.h"
#include "png_host.h"

namespace {

using namespace pf_pngd;

constexpr int PT = 256;
static_assert(PAD_WORDS == PF_PNGD_PAD_WORDS, "pf_hip.h and png_inflate.h disagree");

inline bool words_ok(const uint32_t* words, long nwords, uint32_t nbits) {
  return words && nbits > 0 && nbits <= (1u << 31) && !(reinterpret_cast<uintptr_t>(words) & 3u) && nwords >= (long)((nbits + 31) / 32) + PAD_WORDS;
}

inline int ok() { return hipGetLastError() == hipSuccess ? PF_OK : PF_ERR_LAUNCH; }
#define ST(s) reinterpret_cast<hipStream_t>(s)

__global__ __launch_bounds__(PT) void pngd_find_kernel(const uint32_t* __restrict__ words, uint32_t nbits, uint32_t* __restrict__ list, uint32_t capacity,
                                                       uint32_t* __restrict__ count) {
  const uint64_t g = (uint64_t)blockIdx.x * PT + threadIdx.x;
  if (g >= nbits) return;
  const uint32_t p = (uint32_t)g;
  Bits b(words, nbits);
  const uint32_t type = (peek(b, p) >> 1) & 3u;          // three threads in four leave here
  if (!(type == 2u || (p == 0 && type == 1u))) return;
  if (type == 2u && !probe_dynamic(b, p)) return;
  const uint32_t i = atomicAdd(count, 1u);
  if (i < capacity) list[i] = p;
}

struct WaveCodes {        // one wave's decode state in LDS
  uint8_t lens[MAX_LENS];
  uint16_t lcount[16], lsymbol[288], dcount[16], dsymbol[32], offs[16], lfast[1 << LIT_FAST_BITS], dfast[1 << DIST_FAST_BITS];
  uint32_t head[2];
  __device__ Code lit() { return Code{lcount, lsymbol, lfast, LIT_FAST_BITS}; }
  __device__ Code dist() { return Code{dcount, dsymbol, dfast, DIST_FAST_BITS}; }
};

// Lane 0 reads the header of the block at p and builds the tables; behind the barrier every lane holds the status and the bit of the
// first symbol.  From there all 64 lanes decode the same symbols in step (the same bits, the same table places: nothing diverges), so
// that a match can be spread over the lanes.
__device__ __forceinline__ int wave_block_codes(WaveCodes& wc, const uint32_t* words, uint32_t nbits, uint32_t& p) {
  if (threadIdx.x == 0) {
    Bits b(words, nbits);
    uint32_t q = p;
    wc.head[0] = (uint32_t)(q < nbits ? read_block_codes(b, q, wc.lens, wc.lit(), wc.dist(), wc.offs) : (int)S_EOS);
    wc.head[1] = q;
  }
  __syncthreads();
  p = (uint32_t)__builtin_amdgcn_readfirstlane((int)wc.head[1]);
  return __builtin_amdgcn_readfirstlane((int)wc.head[0]);
}

__global__ __launch_bounds__(64) void pngd_scan_kernel(const uint32_t* __restrict__ words, uint32_t nbits, const uint32_t* __restrict__ starts, int n,
                                                       uint32_t max_bits, uint32_t expected, uint32_t* __restrict__ records) {
  __shared__ WaveCodes wc;
  const int i = blockIdx.x;
  if (i >= n) return;
  Bits b(words, nbits, true);
  const uint32_t start = (uint32_t)__builtin_amdgcn_readfirstlane((int)starts[i]), bfinal = peek(b, start) & 1u;
  uint32_t p = start;
  int st = wave_block_codes(wc, words, nbits, p);
  CountSink sink{0, expected};
  if (st == S_OK) st = decode_symbols(b, p, scan_stop(b, start, max_bits), wc.lit(), wc.dist(), sink);
  if (threadIdx.x == 0) reinterpret_cast<uint4*>(records)[i] = make_uint4(start, p, sink.n, (uint32_t)st | (bfinal << 8));
}

// RefSink of png_inflate.h with a match spread over the wave.  Byte k of a match copies from o - back + k % back, which lies in front of
// the match also where it overlaps itself, so its reference is final and the 64 lanes are independent.  The fence orders this wave's
// earlier stores (one CU, one L1) in front of the loads.
struct WaveRefSink {
  uint8_t* lit;
  uint32_t* ref;
  uint32_t o, base, end;
  __device__ __forceinline__ bool literal(uint8_t v) {
    if (o >= end) return false;
    if (threadIdx.x == 0) {
      lit[o] = v;
      ref[o] = o;
    }
    ++o;
    return true;
  }
  __device__ __forceinline__ int match(uint32_t len, uint32_t back) {
    if (back > o) return S_DIST;
    if (len > end - o) return S_SIZE;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    for (uint32_t k = threadIdx.x; k < len; k += 64) {
      const uint32_t s = o - back + (k < back ? k : k % back);
      ref[o + k] = s >= base ? ref[s] : s;
    }
    o += len;
    return S_OK;
  }
};

__global__ __launch_bounds__(64) void pngd_inflate_kernel(const uint32_t* __restrict__ words, uint32_t nbits, const uint32_t* __restrict__ blocks, int n,
                                                          uint32_t expected, uint8_t* lit, uint32_t* ref, uint32_t* __restrict__ status) {
  __shared__ WaveCodes wc;
  const int i = blockIdx.x;
  if (i >= n) return;
  const uint4 k = reinterpret_cast<const uint4*>(blocks)[i];         // start, type, offset, bytes
  if (k.z > expected || k.w > expected - k.z) {
    if (threadIdx.x == 0) atomicOr(status, (uint32_t)PF_PNGD_F_STREAM);
    return;
  }
  if (k.y == 0) {                                                    // stored: a plain copy, start is a byte offset
    const uint32_t nbytes = nbits >> 3;
    if (k.x > nbytes || k.w > nbytes - k.x) {
      if (threadIdx.x == 0) atomicOr(status, (uint32_t)PF_PNGD_F_STREAM);
      return;
    }
    const uint8_t* src = reinterpret_cast<const uint8_t*>(words) + k.x;
    for (uint32_t j = threadIdx.x; j < k.w; j += 64) {
      lit[k.z + j] = src[j];
      ref[k.z + j] = k.z + j;
    }
    return;
  }
  Bits b(words, nbits, true);
  uint32_t p = (uint32_t)__builtin_amdgcn_readfirstlane((int)k.x);
  int st = wave_block_codes(wc, words, nbits, p);
  const uint32_t off = (uint32_t)__builtin_amdgcn_readfirstlane((int)k.z), len = (uint32_t)__builtin_amdgcn_readfirstlane((int)k.w);
  WaveRefSink sink{lit, ref, off, off, off + len};
  if (st == S_OK) st = decode_symbols(b, p, nbits, wc.lit(), wc.dist(), sink);
  if (threadIdx.x != 0) return;
  if (st == S_DIST) atomicOr(status, (uint32_t)PF_PNGD_F_DISTANCE);
  else if (st != S_OK || sink.o != sink.end) atomicOr(status, (uint32_t)PF_PNGD_F_STREAM);
}

__global__ __launch_bounds__(PT) void pngd_jump_kernel(uint32_t* ref, uint32_t n) {
  const uint64_t i = (uint64_t)blockIdx.x * PT + threadIdx.x;
  if (i >= n) return;
  const uint32_t a = ref[i];
  if (a >= i) return;                       // a literal (a == i; a > i never is stored)
  const uint32_t c = ref[a];
  if (c < a) ref[i] = c;
}

__global__ __launch_bounds__(PT) void pngd_gather_kernel(const uint8_t* __restrict__ lit, const uint32_t* __restrict__ ref, uint32_t n,
                                                         uint8_t* __restrict__ out) {
  const uint64_t i = (uint64_t)blockIdx.x * PT + threadIdx.x;
  if (i >= n) return;
  const uint32_t a = ref[i];
  out[i] = lit[a <= i ? a : (uint32_t)i];
}

// ---- Adler-32: A = 1 + sum d_i, B = n + sum (n - i) d_i, both mod 65521; 16 bytes per thread, 64-bit sums
__global__ __launch_bounds__(PT) void pngd_adler_kernel(const uint8_t* __restrict__ data, long n, unsigned long long* __restrict__ sums) {
  const long i0 = ((long)blockIdx.x * PT + threadIdx.x) * 16;
  unsigned long long sa = 0, sb = 0;
  if (i0 < n) {
    uint32_t s = 0, t = 0;
    if (i0 + 16 <= n) {
      const uint4 v = *reinterpret_cast<const uint4*>(data + i0);
      const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        const uint32_t d = (w[k >> 2] >> (8 * (k & 3))) & 255u;
        s += d;
        t += (uint32_t)k * d;
      }
    } else {
      for (int k = 0; i0 + k < n; ++k) {
        s += data[i0 + k];
        t += (uint32_t)k * data[i0 + k];
      }
    }
    sa = s;
    sb = ((unsigned long long)((n - i0) % 65521) + 65521ull) * s - t;       // = sum (n - i0 - k) d_k mod 65521, never negative
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    sa += __shfl_xor(sa, o, 64);
    sb += __shfl_xor(sb, o, 64);
  }
  if ((threadIdx.x & 63) == 0 && (sa | sb)) {
    atomicAdd(sums, sa);
    atomicAdd(sums + 1, sb);
  }
}

__global__ void pngd_adler_final_kernel(const unsigned long long* __restrict__ sums, long n, uint32_t* __restrict__ result) {
  const uint32_t a = (uint32_t)((1ull + sums[0]) % 65521ull), b = (uint32_t)(((unsigned long long)(n % 65521) + sums[1]) % 65521ull);
  result[0] = (b << 16) | a;
}

// ---- unfilter
template <int BPP, int NR>
__global__ __launch_bounds__(64) void pngd_unfilter_kernel(const uint8_t* __restrict__ inf, int H, long rowbytes, uint8_t* __restrict__ recon,
                                                           uint32_t* __restrict__ status) {
  constexpr int TILE = 64 * BPP, PITCH = 2 * TILE + ((4 + BPP) & 7);      // lanes one row and one pixel apart fall on different banks
  __shared__ uint8_t ring[NR + 1][PITCH];
  const int lane = threadIdx.x;
  const long stride = rowbytes + 1;
  const int r0 = blockIdx.x;
  const uint32_t f0 = inf[r0 * stride];
  if (r0 != 0 && f0 >= 2 && f0 <= 4) return;          // this row continues the run above it
  int r1 = H;                                          // the run ends in front of the next row that needs nothing from above
  for (int base = r0 + 1; base < H; base += 64) {
    const int row = base + lane;
    bool starts = true;
    if (row < H) {
      const uint32_t f = inf[row * stride];
      starts = !(f >= 2 && f <= 4);
    }
    const unsigned long long m = __ballot(starts);
    if (m) {
      r1 = min(H, base + __ffsll(m) - 1);
      break;
    }
  }
  const long npix = rowbytes / BPP, ntiles = (npix + 63) / 64;
  for (int rb = r0; rb < r1; rb += NR) {
    const int nrows = min(NR, r1 - rb);
    const bool active = lane < nrows;
    uint32_t ft = active ? inf[(rb + lane) * stride] : 0u;
    if (ft > 4u) {
      atomicOr(status, (uint32_t)PF_PNGD_F_FILTER);
      ft = 0;
    }
    uint32_t a[BPP], c[BPP];
#pragma unroll
    for (int k = 0; k < BPP; ++k) a[k] = c[k] = 0;
    for (long m = 0; m <= ntiles; ++m) {
      if (m < ntiles) {                                // tile m of the band (and of the row above it) into ring slot m & 1
        const long x0 = 64 * m;
        const int nb = (int)min(64l, npix - x0) * BPP, slot = (int)(m & 1) * TILE;
        for (int j = lane; j < nb; j += 64) ring[0][slot + j] = rb > r0 ? recon[(rb - 1) * rowbytes + x0 * BPP + j] : (uint8_t)0;
        for (int rr = 0; rr < nrows; ++rr)
          for (int j = lane; j < nb; j += 64) ring[rr + 1][slot + j] = inf[(rb + rr) * stride + 1 + x0 * BPP + j];
      }
      __syncthreads();
      for (int s = 0; s < 64; ++s) {
        const long x = 64 * m + s - lane;
        if (active && x >= 0 && x < npix) {
          const int col = (int)(x & 127) * BPP;
#pragma unroll
          for (int k = 0; k < BPP; ++k) {
            const uint32_t f = ring[lane + 1][col + k], b = ring[lane][col + k];
            uint32_t pred = 0;
            if (ft == 1u) pred = a[k];
            else if (ft == 2u) pred = b;
            else if (ft == 3u) pred = (a[k] + b) >> 1;
            else if (ft == 4u) {
              const int pa = abs((int)b - (int)c[k]), pb = abs((int)a[k] - (int)c[k]), pc = abs((int)a[k] + (int)b - 2 * (int)c[k]);
              pred = (pa <= pb && pa <= pc) ? a[k] : (pb <= pc ? b : c[k]);
            }
            const uint32_t v = (f + pred) & 255u;
            ring[lane + 1][col + k] = (uint8_t)v;
            a[k] = v;
            c[k] = b;
          }
        }
        // lane l + 1 reads at the next step what lane l stored at this one: keep the order of the LDS accesses across the step
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
      }
      __syncthreads();
      if (m >= 1) {                                    // tile m - 1 is finished in every row
        const long x0 = 64 * (m - 1);
        const int nb = (int)min(64l, npix - x0) * BPP, slot = (int)((m - 1) & 1) * TILE;
        for (int rr = 0; rr < nrows; ++rr)
          for (int j = lane; j < nb; j += 64) recon[(rb + rr) * rowbytes + x0 * BPP + j] = ring[rr + 1][slot + j];
      }
    }
    __syncthreads();                                   // the band's last row is read back as the next band's row above
  }
}

// ---- expand: the layouts that differ from the unfiltered rows
__global__ __launch_bounds__(PT) void pngd_expand_bits_kernel(const uint8_t* __restrict__ recon, int H, int W, long rowbytes, int depth, int palette_entries,
                                                              const uint8_t* __restrict__ palette, uint8_t* __restrict__ out,
                                                              uint32_t* __restrict__ status) {
  const long i = (long)blockIdx.x * PT + threadIdx.x;
  if (i >= (long)H * W) return;
  const long y = i / W, x = i % W;
  const long bit = x * depth;
  uint32_t v = (recon[y * rowbytes + (bit >> 3)] >> (8 - depth - (int)(bit & 7))) & ((1u << depth) - 1u);
  if (palette) {                                        // colour type 3 -> RGB
    if (v >= (uint32_t)palette_entries) {
      atomicOr(status, (uint32_t)PF_PNGD_F_PLTE);
      v = 0;
    }
    out[3 * i] = palette[3 * v];
    out[3 * i + 1] = palette[3 * v + 1];
    out[3 * i + 2] = palette[3 * v + 2];
  } else {                                              // grey of 1 / 2 / 4 bits: bit replication
    out[i] = (uint8_t)(v * (255u / ((1u << depth) - 1u)));
  }
}

__global__ __launch_bounds__(PT) void pngd_expand_16_kernel(const uint8_t* __restrict__ recon, long samples, uint16_t* __restrict__ out) {
  const long i = (long)blockIdx.x * PT + threadIdx.x;
  if (i < samples) out[i] = (uint16_t)((recon[2 * i] << 8) | recon[2 * i + 1]);
}

template <typename T>
__global__ __launch_bounds__(PT) void pngd_to_rgb8_kernel(const T* __restrict__ in, long pixels, int channels, uint8_t* __restrict__ rgb) {
  const long i = (long)blockIdx.x * PT + threadIdx.x;
  if (i >= pixels) return;
  constexpr int SH = 8 * (sizeof(T) - 1);               // strip_16: the high byte
  const T* p = in + i * channels;
  const bool colour = channels >= 3;
  rgb[3 * i] = (uint8_t)(p[0] >> SH);
  rgb[3 * i + 1] = (uint8_t)(p[colour ? 1 : 0] >> SH);
  rgb[3 * i + 2] = (uint8_t)(p[colour ? 2 : 0] >> SH);
}

inline bool header_ok(const pf_pngd_header* h) {
  if (!h || h->width < 1 || h->height < 1 || h->interlace) return false;
  const int ct = h->color_type, d = h->depth;
  const bool ok = (ct == 0 && (d == 1 || d == 2 || d == 4 || d == 8 || d == 16)) || (ct == 3 && (d == 1 || d == 2 || d == 4 || d == 8)) ||
                  ((ct == 2 || ct == 4 || ct == 6) && (d == 8 || d == 16));
  if (!ok || h->channels != channels_of(ct)) return false;
  const int bits = h->channels * d;
  return h->bpp == (bits < 8 ? 1 : bits / 8) && h->rowbytes == ((int64_t)h->width * bits + 7) / 8 &&
         h->inflated_bytes == (int64_t)h->height * (1 + h->rowbytes) && h->plte_entries >= 0 && h->plte_entries <= 256;
}

inline unsigned blocks_for(long n) { return (unsigned)((n + PT - 1) / PT); }

}  // namespace

// ---- host-only steps: no GPU call
extern "C" int pf_pngd_parse(const uint8_t* data, long len, int check_idat_crc, pf_pngd_header* header, uint8_t* deflate, long capacity,
                             long* deflate_len) {
  return pf_pngd::parse(data, len, check_idat_crc, header, deflate, capacity, deflate_len);
}
extern "C" int pf_pngd_find_host(const uint32_t* words, long nwords, uint32_t nbits, uint32_t* list, long capacity, long* count) {
  if (!words_ok(words, nwords, nbits) || !list || !count || capacity < 0) return PF_ERR_ARG;
  Bits b(words, nbits);
  long n = 0;
  for (uint32_t p = 0; p < nbits; ++p) {
    const uint32_t type = (peek(b, p) >> 1) & 3u;
    if (!((p == 0 && type == 1u) || (type == 2u && probe_dynamic(b, p)))) continue;
    if (n < capacity) list[n] = p;
    ++n;
  }
  *count = n;
  return PF_OK;
}
extern "C" int pf_pngd_scan_host(const uint32_t* words, long nwords, uint32_t nbits, const uint32_t* starts, int n, uint32_t max_block_bits, uint32_t expected,
                                 uint32_t* records) {
  if (!words_ok(words, nwords, nbits) || !starts || !records || n < 0) return PF_ERR_ARG;
  HostCodes hc;
  for (int i = 0; i < n; ++i)
    scan_block(Bits(words, nbits), starts[i], max_block_bits, expected, hc.lens, hc.lit(), hc.dist(), hc.offs, records + 4 * (long)i);
  return PF_OK;
}
extern "C" int pf_pngd_inflate_model_host(const uint8_t* deflate, long len, long expected, uint32_t max_block_bits, uint8_t* out, long* stats) {
  if (!deflate || !out) return PF_ERR_ARG;
  return inflate_model(deflate, len, expected, max_block_bits, out, stats);
}

// ---- device steps
extern "C" int pf_pngd_find(const uint32_t* words, long nwords, uint32_t nbits, uint32_t* list, uint32_t capacity, uint32_t* count, void* stream) {
  if (!words_ok(words, nwords, nbits) || !list || !count) return PF_ERR_ARG;
  if (hipMemsetAsync(count, 0, 4, ST(stream)) != hipSuccess) return PF_ERR_LAUNCH;
  hipLaunchKernelGGL(pngd_find_kernel, dim3(blocks_for(nbits)), dim3(PT), 0, ST(stream), words, nbits, list, capacity, count);
  return ok();
}

extern "C" int pf_pngd_scan(const uint32_t* words, long nwords, uint32_t nbits, const uint32_t* starts, int n, uint32_t max_block_bits, uint32_t expected,
                            uint32_t* records, void* stream) {
  if (!words_ok(words, nwords, nbits) || !starts || !records || n < 0 || (reinterpret_cast<uintptr_t>(records) & 15u))
    return PF_ERR_ARG;
  if (n == 0) return PF_OK;
  hipLaunchKernelGGL(pngd_scan_kernel, dim3(n), dim3(64), 0, ST(stream), words, nbits, starts, n, max_block_bits, expected, records);
  return ok();
}

extern "C" int pf_pngd_inflate(const uint32_t* words, long nwords, uint32_t nbits, const uint32_t* blocks, int nblocks, uint32_t expected, uint8_t* lit,
                               uint32_t* ref, uint32_t* status, void* stream) {
  if (!words_ok(words, nwords, nbits) || !blocks || !lit || !ref || !status || nblocks < 1 || expected == 0 ||
      expected > 0x7fffffffu || (reinterpret_cast<uintptr_t>(blocks) & 15u))
    return PF_ERR_ARG;
  hipLaunchKernelGGL(pngd_inflate_kernel, dim3(nblocks), dim3(64), 0, ST(stream), words, nbits, blocks, nblocks, expected, lit, ref, status);
  return ok();
}

extern "C" int pf_pngd_resolve(const uint8_t* lit, uint32_t* ref, uint32_t n, int rounds, uint8_t* out, void* stream) {
  if (!lit || !ref || !out || n == 0 || n > 0x7fffffffu || rounds < 0 || rounds > 33) return PF_ERR_ARG;
  for (int r = 0; r < rounds; ++r) hipLaunchKernelGGL(pngd_jump_kernel, dim3(blocks_for(n)), dim3(PT), 0, ST(stream), ref, n);
  hipLaunchKernelGGL(pngd_gather_kernel, dim3(blocks_for(n)), dim3(PT), 0, ST(stream), lit, ref, n, out);
  return ok();
}

extern "C" int pf_pngd_adler(const uint8_t* data, long n, uint64_t* sums, uint32_t* result, void* stream) {
  if (!data || !sums || !result || n < 1 || (reinterpret_cast<uintptr_t>(data) & 15u) || (reinterpret_cast<uintptr_t>(sums) & 7u))
    return PF_ERR_ARG;
  if (hipMemsetAsync(sums, 0, 16, ST(stream)) != hipSuccess) return PF_ERR_LAUNCH;
  hipLaunchKernelGGL(pngd_adler_kernel, dim3(blocks_for((n + 15) / 16)), dim3(PT), 0, ST(stream), data, n,
                     reinterpret_cast<unsigned long long*>(sums));
  hipLaunchKernelGGL(pngd_adler_final_kernel, dim3(1), dim3(1), 0, ST(stream), reinterpret_cast<const unsigned long long*>(sums), n, result);
  return ok();
}

extern "C" int pf_pngd_unfilter(const uint8_t* inflated, const pf_pngd_header* header, uint8_t* recon, uint32_t* status, void* stream) {
  if (!header_ok(header) || !inflated || !recon || !status) return PF_ERR_ARG;
  const int H = header->height;
  const long rb = header->rowbytes;
#define PF_PNGD_UNFILTER(BPP, NR) \
  hipLaunchKernelGGL((pngd_unfilter_kernel<BPP, NR>), dim3(H), dim3(64), 0, ST(stream), inflated, H, rb, recon, status)
  switch (header->bpp) {
    case 1: PF_PNGD_UNFILTER(1, 64); break;
    case 2: PF_PNGD_UNFILTER(2, 64); break;
    case 3: PF_PNGD_UNFILTER(3, 64); break;
    case 4: PF_PNGD_UNFILTER(4, 64); break;
    case 6: PF_PNGD_UNFILTER(6, 32); break;
    case 8: PF_PNGD_UNFILTER(8, 32); break;
    default: return PF_ERR_ARG;
  }
#undef PF_PNGD_UNFILTER
  return ok();
}

extern "C" int pf_pngd_expand(const uint8_t* recon, const pf_pngd_header* header, const uint8_t* palette, void* image, uint32_t* status,
                              void* stream) {
  if (!header_ok(header) || !recon || !image || !status) return PF_ERR_ARG;
  const long pixels = (long)header->height * header->width;
  if (header->depth == 16) {
    if (reinterpret_cast<uintptr_t>(image) & 1u) return PF_ERR_ARG;
    const long samples = pixels * header->channels;
    hipLaunchKernelGGL(pngd_expand_16_kernel, dim3(blocks_for(samples)), dim3(PT), 0, ST(stream), recon, samples, static_cast<uint16_t*>(image));
  } else if (header->color_type == 3 || header->depth < 8) {
    const bool pal = header->color_type == 3;
    if (pal && (!palette || header->plte_entries < 1)) return PF_ERR_ARG;
    hipLaunchKernelGGL(pngd_expand_bits_kernel, dim3(blocks_for(pixels)), dim3(PT), 0, ST(stream), recon, header->height, header->width,
                       (long)header->rowbytes, header->depth, header->plte_entries, pal ? palette : nullptr, static_cast<uint8_t*>(image), status);
  } else {
    return PF_ERR_ARG;               // 8-bit grey, grey+alpha, RGB and RGBA rows are the image already
  }
  return ok();
}

extern "C" int pf_pngd_to_rgb8(const void* image, int height, int width, int channels, int bits, uint8_t* rgb, void* stream) {
  if (!image || !rgb || height < 1 || width < 1 || channels < 1 || channels > 4 || (bits != 8 && bits != 16)) return PF_ERR_ARG;
  const long pixels = (long)height * width;
  if (bits == 16)
    hipLaunchKernelGGL(pngd_to_rgb8_kernel<uint16_t>, dim3(blocks_for(pixels)), dim3(PT), 0, ST(stream), static_cast<const uint16_t*>(image), pixels,
                       channels, rgb);
  else
    hipLaunchKernelGGL(pngd_to_rgb8_kernel<uint8_t>, dim3(blocks_for(pixels)), dim3(PT), 0, ST(stream), static_cast<const uint8_t*>(image), pixels,
                       channels, rgb);
  return ok();
}
