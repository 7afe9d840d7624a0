// PNG inflate with the symbols of a block decoded in parallel subsequences (include/pf_hip.h, "PNG decoding"; the opt-in
// block_decode='subsequences' of preprocess.decode_png).  csrc/png_decode.hip gives a block to one wave, which decodes one symbol after
// the other; here a block goes to one workgroup of PAR_WINDOW threads, and every thread decodes one lane, S bits of the stream, from a
// guessed entry.  Deflate self-synchronises: a decoder started at an arbitrary bit soon meets a true code boundary, so after a few rounds
// of "decode again from where my predecessor ended" every lane starts at its true entry (png_inflate.h states the scheme and holds the
// lane decoder, which the host models of png_host.h run through the same schedule).  A round reads only the exits of the round before
// (double-buffered in LDS), so the number of rounds is a property of the file, S and PAR_WINDOW, not of the thread schedule.
//
// Scan: one workgroup per candidate; the rounds per window, then the true chain's end bit and byte total: the record of pngd_scan_kernel
// wherever that one's status is S_OK.  Inflate: one workgroup per true block; the same rounds, an exclusive sum of the lanes' byte counts
// gives each lane its output range, and each lane of the true chain decodes once more from its final entry into lit / ref.  A matched
// byte takes ref[source] when the source lies in the lane's own range (written by the same thread) and the source itself otherwise, so
// after the pass a reference points to a literal or into a strictly earlier lane's range, and pf_pngd_resolve finishes as before.
//
// Termination and bounds (the invariants of png_decode.hip, kept here):
//   * no kernel waits on a word another workgroup writes: only workgroup barriers are used, and the two max / or words in global memory
//     are written with atomics and never read;
//   * every barrier is reached by all threads: the window loop, the round loop and every early exit depend only on kernel arguments,
//     on values all threads read from LDS behind a barrier, or on the result of a barrier-wide reduction;
//   * every bit read goes through peek(): 0 at or past nbits, otherwise inside the zero-padded buffer the entry points check;
//   * every loop over file data has a bound that is not data: a lane turns while p < end <= nbits and consumes at least one bit per
//     turn; the rounds of a window are fewer than its lanes, at most PAR_WINDOW; the windows of a block at most nbits / (S * PAR_WINDOW) + 1;
//   * the scan pass stores only its own record; the inflate pass stores lit[o] and ref[o] only for o inside its block's
//     [offset, offset + bytes), checked against the expected size first, and inside the storing lane's own range, which no other lane
//     writes; a match source is checked against the start of the output; ref[o] <= o always.
#include "pf_common.h"
#include "../../include/pf_hip.h"
#include "png_host.h"

namespace {

using namespace pf_pngd;

constexpr int T = PAR_WINDOW, WAVES = T / 64;
static_assert(T % 64 == 0 && T >= 64 && T <= 1024, "a window is a workgroup of whole waves");
static_assert(PAD_WORDS == PF_PNGD_PAD_WORDS, "pf_hip.h and png_inflate.h disagree");

inline bool words_ok(const uint32_t* words, long nwords, uint32_t nbits) {
  return words && nbits > 0 && nbits <= (1u << 31) && !(reinterpret_cast<uintptr_t>(words) & 3u) && nwords >= (long)((nbits + 31) / 32) + PAD_WORDS;
}

inline int ok() { return hipGetLastError() == hipSuccess ? PF_OK : PF_ERR_LAUNCH; }
#define ST(s) reinterpret_cast<hipStream_t>(s)

struct ParShared {        // one workgroup's state in LDS: the block's tables, the double-buffered exits, what the chain comes to
  uint8_t lens[MAX_LENS];
  uint16_t lcount[16], lsymbol[288], dcount[16], dsymbol[32], offs[16], lfast[1 << LIT_FAST_BITS], dfast[1 << DIST_FAST_BITS];
  uint32_t head[2];
  uint32_t exit[2][T];
  uint8_t eob[2][T];
  unsigned long long wave_sum[WAVES], total;
  int first_eob, first_inv, first_size;
  uint32_t carry;
  __device__ Code lit() { return Code{lcount, lsymbol, lfast, LIT_FAST_BITS}; }
  __device__ Code dist() { return Code{dcount, dsymbol, dfast, DIST_FAST_BITS}; }
};

// Thread 0 reads the header of the block at p and builds the tables; behind the barrier every thread holds the status and the bit of
// the first symbol.
__device__ __forceinline__ int block_codes(ParShared& sh, const uint32_t* words, uint32_t nbits, uint32_t& p) {
  if (threadIdx.x == 0) {
    Bits b(words, nbits);
    uint32_t q = p;
    sh.head[0] = (uint32_t)(q < nbits ? read_block_codes(b, q, sh.lens, sh.lit(), sh.dist(), sh.offs) : (int)S_EOS);
    sh.head[1] = q;
  }
  __syncthreads();
  p = sh.head[1];
  return (int)sh.head[0];
}

// The rounds of one window.  Thread k is lane `first + k`; lane 0 enters at `carry`.  -> the lane as it is final, its entry in `entry`,
// in `rounds` the number of rounds in which some lane changed (the same in every thread).
__device__ __forceinline__ Lane window_rounds(ParShared& sh, Bits& b, uint32_t first, uint32_t carry, uint32_t stop, uint32_t S, uint32_t& entry,
                                              uint32_t& rounds, int& live) {
  const int k = threadIdx.x;
  live = lanes_in_window(first, S, stop);
  const uint32_t end = lane_end(first + (uint32_t)k, S, stop);
  const Code lit = sh.lit(), dist = sh.dist();
  NullSink null;
  entry = k == 0 ? carry : (first + (uint32_t)k) * S;
  Lane l{entry, 0u, 0u, 0u, S_OK};
  if (k < live) l = decode_lane(b, entry, end, lit, dist, null);
  sh.exit[0][k] = l.exit;
  sh.eob[0][k] = (uint8_t)(l.flags & L_EOB);
  if (k == 0) sh.first_eob = sh.first_inv = sh.first_size = T;
  __syncthreads();
  rounds = 0;
  for (int r = 1; r < live; ++r) {
    const int from = (r - 1) & 1, to = r & 1;
    int changed = 0;
    if (k > 0 && k < live && !sh.eob[from][k - 1] && sh.exit[from][k - 1] != entry) {
      entry = sh.exit[from][k - 1];
      l = decode_lane(b, entry, end, lit, dist, null);
      changed = 1;
    }
    sh.exit[to][k] = l.exit;
    sh.eob[to][k] = (uint8_t)(l.flags & L_EOB);
    if (!__syncthreads_or(changed)) break;
    rounds = (uint32_t)r;
  }
  return l;
}

// Inclusive sum of v over the workgroup, in front of it `base`; behind the call sh.total holds base + the sum of all.  Two barriers.
__device__ __forceinline__ unsigned long long window_sum(ParShared& sh, unsigned long long base, uint32_t v) {
  const int k = threadIdx.x, lane = k & 63, wave = k >> 6;
  unsigned long long s = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned long long t = __shfl_up(s, o, 64);
    if (lane >= o) s += t;
  }
  if (lane == 63) sh.wave_sum[wave] = s;
  __syncthreads();
  unsigned long long before = base, all = base;
  for (int i = 0; i < WAVES; ++i) {
    const unsigned long long t = sh.wave_sum[i];
    if (i < wave) before += t;
    all += t;
  }
  if (k == 0) sh.total = all;
  __syncthreads();
  return before + s;
}

__global__ __launch_bounds__(T) void pngd_scan_par_kernel(const uint32_t* __restrict__ words, uint32_t nbits, const uint32_t* __restrict__ starts, int n,
                                                          uint32_t max_bits, uint32_t expected, uint32_t S, uint32_t* __restrict__ records,
                                                          uint32_t* __restrict__ max_rounds) {
  __shared__ ParShared sh;
  const int i = blockIdx.x, k = threadIdx.x;
  if (i >= n) return;
  Bits b(words, nbits);
  const uint32_t start = starts[i], bfinal = peek(b, start) & 1u;
  uint32_t p = start, most = 0;
  unsigned long long total = 0;
  int st = block_codes(sh, words, nbits, p);
  if (st == S_OK) {
    const uint32_t stop = scan_stop(b, start, max_bits);
    st = stop >= nbits ? S_EOS : S_LIMIT;
    for (uint32_t first = p / S; (uint64_t)first * S < stop; first += T) {
      uint32_t entry, rounds;
      int live;
      const Lane l = window_rounds(sh, b, first, p, stop, S, entry, rounds, live);
      most = max(most, rounds);
      const unsigned long long incl = window_sum(sh, total, l.bytes);
      if (l.flags & L_EOB) atomicMin(&sh.first_eob, k);
      if (l.flags & L_INVALID) atomicMin(&sh.first_inv, k);
      if (incl > expected) atomicMin(&sh.first_size, k);
      __syncthreads();
      int how;
      const int at = chain_event(sh.first_eob, sh.first_inv, sh.first_size, how);
      if (k == (at < T ? at : live - 1)) {
        sh.carry = (at < T && how == S_OK) ? l.eob : l.exit;
        if (at < T) sh.total = incl;
      }
      __syncthreads();
      p = sh.carry;
      total = sh.total;
      if (at < T) {
        st = how == S_OK ? (p > nbits ? S_EOS : S_OK) : how;
        break;
      }
    }
  }
  if (k != 0) return;
  reinterpret_cast<uint4*>(records)[i] = make_uint4(start, p, total > 0xffffffffull ? 0xffffffffu : (uint32_t)total, (uint32_t)st | (bfinal << 8));
  if (most) atomicMax(max_rounds, most);
}

__global__ __launch_bounds__(T) void pngd_inflate_par_kernel(const uint32_t* __restrict__ words, uint32_t nbits, const uint32_t* __restrict__ blocks, int n,
                                                             uint32_t expected, uint32_t S, uint8_t* lit, uint32_t* ref, uint32_t* __restrict__ status,
                                                             uint32_t* __restrict__ max_rounds) {
  __shared__ ParShared sh;
  const int i = blockIdx.x, k = threadIdx.x;
  if (i >= n) return;
  const uint4 blk = reinterpret_cast<const uint4*>(blocks)[i];       // start, type, offset, bytes
  if (blk.z > expected || blk.w > expected - blk.z) {
    if (k == 0) atomicOr(status, (uint32_t)PF_PNGD_F_STREAM);
    return;
  }
  if (blk.y == 0) {                                                  // stored: a plain copy, start is a byte offset
    const uint32_t nbytes = nbits >> 3;
    if (blk.x > nbytes || blk.w > nbytes - blk.x) {
      if (k == 0) atomicOr(status, (uint32_t)PF_PNGD_F_STREAM);
      return;
    }
    const uint8_t* src = reinterpret_cast<const uint8_t*>(words) + blk.x;
    for (uint32_t j = k; j < blk.w; j += T) {
      lit[blk.z + j] = src[j];
      ref[blk.z + j] = blk.z + j;
    }
    return;
  }
  Bits b(words, nbits);
  uint32_t p = blk.x, most = 0, flags = 0;
  const uint32_t off = blk.z, end = blk.z + blk.w;
  unsigned long long total = 0;
  bool ended = false;
  if (block_codes(sh, words, nbits, p) == S_OK) {
    for (uint32_t first = p / S; (uint64_t)first * S < nbits; first += T) {
      uint32_t entry, rounds;
      int live;
      const Lane l = window_rounds(sh, b, first, p, nbits, S, entry, rounds, live);
      most = max(most, rounds);
      const unsigned long long incl = window_sum(sh, total, l.bytes);
      if (l.flags & L_EOB) atomicMin(&sh.first_eob, k);
      __syncthreads();
      const int e = sh.first_eob;
      if (k <= e && k < live) {                                      // the true chain: once more, storing
        const unsigned long long at = (unsigned long long)off + (incl - l.bytes);
        const uint32_t o = at < end ? (uint32_t)at : end;
        RefSink sink{lit, ref, o, o, end};
        const Lane again = decode_lane(b, entry, lane_end(first + (uint32_t)k, S, nbits), sh.lit(), sh.dist(), sink);
        if (again.sink == S_DIST) flags |= PF_PNGD_F_DISTANCE;
        else if (again.sink != S_OK || (again.flags & L_INVALID)) flags |= PF_PNGD_F_STREAM;
      }
      if (k == (e < T ? e : live - 1)) {
        sh.carry = l.exit;
        if (e < T) sh.total = incl;
      }
      __syncthreads();
      p = sh.carry;
      total = sh.total;
      if (e < T) {
        ended = true;
        break;
      }
    }
  }
  if (k == 0 && (!ended || (unsigned long long)off + total != end)) flags |= PF_PNGD_F_STREAM;
  if (flags) atomicOr(status, flags);
  if (k == 0 && most) atomicMax(max_rounds, most);
}

inline bool scan_args_ok(const uint32_t* words, long nwords, uint32_t nbits, const uint32_t* starts, int n, const uint32_t* records, uint32_t S,
                         const uint32_t* max_rounds) {
  return words_ok(words, nwords, nbits) && starts && records && n >= 0 && par_bits_ok(S) && max_rounds;
}
inline bool inflate_args_ok(const uint32_t* words, long nwords, uint32_t nbits, const uint32_t* blocks, int nblocks, uint32_t expected, const uint8_t* lit,
                            const uint32_t* ref, const uint32_t* status, uint32_t S, const uint32_t* max_rounds) {
  return words_ok(words, nwords, nbits) && blocks && lit && ref && status && nblocks >= 1 && expected != 0 && expected <= 0x7fffffffu && par_bits_ok(S) &&
         max_rounds;
}

}  // namespace

extern "C" int pf_pngd_par_window(void) { return PAR_WINDOW; }

// ---- host models: no GPU call.  max_rounds is raised, never lowered, as the device entries do.
extern "C" int pf_pngd_scan_par_host(const uint32_t* words, long nwords, uint32_t nbits, const uint32_t* starts, int n, uint32_t max_block_bits,
                                     uint32_t expected, uint32_t subsequence_bits, uint32_t* records, uint32_t* max_rounds) {
  if (!scan_args_ok(words, nwords, nbits, starts, n, records, subsequence_bits, max_rounds)) return PF_ERR_ARG;
  HostCodes hc;
  std::vector<ParWindowHost> w(1);
  for (int i = 0; i < n; ++i) {
    const uint32_t r = scan_block_par(Bits(words, nbits), starts[i], max_block_bits, expected, subsequence_bits, hc, w[0], records + 4 * (long)i);
    if (r > *max_rounds) *max_rounds = r;
  }
  return PF_OK;
}

extern "C" int pf_pngd_inflate_par_host(const uint32_t* words, long nwords, uint32_t nbits, const uint32_t* blocks, int nblocks, uint32_t expected,
                                        uint32_t subsequence_bits, uint8_t* lit, uint32_t* ref, uint32_t* status, uint32_t* max_rounds) {
  if (!inflate_args_ok(words, nwords, nbits, blocks, nblocks, expected, lit, ref, status, subsequence_bits, max_rounds)) return PF_ERR_ARG;
  HostCodes hc;
  std::vector<ParWindowHost> w(1);
  const uint32_t nbytes = nbits >> 3;
  for (int i = 0; i < nblocks; ++i) {
    const uint32_t* k = blocks + 4 * (long)i;
    if (k[2] > expected || k[3] > expected - k[2]) {
      *status |= PF_PNGD_F_STREAM;
      continue;
    }
    if (k[1] == 0) {
      if (k[0] > nbytes || k[3] > nbytes - k[0]) {
        *status |= PF_PNGD_F_STREAM;
        continue;
      }
      const uint8_t* src = reinterpret_cast<const uint8_t*>(words) + k[0];
      for (uint32_t j = 0; j < k[3]; ++j) {
        lit[k[2] + j] = src[j];
        ref[k[2] + j] = k[2] + j;
      }
      continue;
    }
    *status |= inflate_block_par(Bits(words, nbits), k, subsequence_bits, hc, w[0], lit, ref, max_rounds);
  }
  return PF_OK;
}

// ---- device steps
extern "C" int pf_pngd_scan_par(const uint32_t* words, long nwords, uint32_t nbits, const uint32_t* starts, int n, uint32_t max_block_bits, uint32_t expected,
                                uint32_t subsequence_bits, uint32_t* records, uint32_t* max_rounds, void* stream) {
  if (!scan_args_ok(words, nwords, nbits, starts, n, records, subsequence_bits, max_rounds) || (reinterpret_cast<uintptr_t>(records) & 15u) ||
      (reinterpret_cast<uintptr_t>(max_rounds) & 3u))
    return PF_ERR_ARG;
  if (n == 0) return PF_OK;
  hipLaunchKernelGGL(pngd_scan_par_kernel, dim3(n), dim3(T), 0, ST(stream), words, nbits, starts, n, max_block_bits, expected, subsequence_bits, records,
                     max_rounds);
  return ok();
}

extern "C" int pf_pngd_inflate_par(const uint32_t* words, long nwords, uint32_t nbits, const uint32_t* blocks, int nblocks, uint32_t expected,
                                   uint32_t subsequence_bits, uint8_t* lit, uint32_t* ref, uint32_t* status, uint32_t* max_rounds, void* stream) {
  if (!inflate_args_ok(words, nwords, nbits, blocks, nblocks, expected, lit, ref, status, subsequence_bits, max_rounds) ||
      (reinterpret_cast<uintptr_t>(blocks) & 15u) || (reinterpret_cast<uintptr_t>(max_rounds) & 3u))
    return PF_ERR_ARG;
  hipLaunchKernelGGL(pngd_inflate_par_kernel, dim3(nblocks), dim3(T), 0, ST(stream), words, nbits, blocks, nblocks, expected, subsequence_bits, lit, ref,
                     status, max_rounds);
  return ok();
}
