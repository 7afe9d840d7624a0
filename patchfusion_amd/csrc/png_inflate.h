// The deflate pieces the PNG decoder runs on both sides (csrc/png_decode.hip on the device, csrc/png_host.h and tests/host/png_decode_main.cpp
// on the host): the bit reader, the dynamic-header test of the block finder, the header reader, the canonical-code build and the symbol
// loop.  No GPU header and no library call: every array is handed in by the caller (LDS on the device, the stack on the host).
//
// Bounds, relied on by every user:
//   * Bits.w holds (nbits + 31) / 32 + PAD_WORDS words, zero past the stream; peek() returns 0 for p >= nbits and otherwise reads
//     words p / 32 .. p / 32 + PAD_WORDS - 1, all inside;
//   * decode_sym reads fast[j] with j < 1 << fast_bits, count[1..15] and symbol[j] with j < the number of symbols of non-zero length
//     (j = index + code - first, code - first < count[len]); build_code fills fast only for a code that is not over-subscribed, so
//     the walk over its codes stays inside symbol[];
//   * read_dynamic_header writes lens[i] only for i < nlit + ndist <= 316;
//   * decode_symbols consumes at least one bit per turn and turns only while p < stop, so it is bounded by stop - p on entry; what a
//     symbol stores is checked by the sink against the expected size before the store.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PF_PNGD_HD __host__ __device__ __forceinline__
#else
#define PF_PNGD_HD inline
#endif

namespace pf_pngd {

enum { S_OK = 0, S_INVALID = 1, S_LIMIT = 2, S_EOS = 3, S_SIZE = 4, S_DIST = 5 };   // how a block's decode ended
constexpr int MAX_LENS = 320;          // 288 literal/length + 32 distance code lengths

constexpr int PAD_WORDS = 2;             // zero words behind the stream: what the window may touch

struct Bits {
  const uint32_t* w;      // the deflate stream as little-endian words, zero padded (see above)
  uint32_t nbits;
  // a two-word window over the stream, lo = w[wi] and hi = w[wi + 1]: a decoder moves forward, so most symbols come out of registers
  uint32_t wi = 0xfffffffeu, lo = 0, hi = 0;      // no word index is 2^32 - 2 or follows it
  // device only: every lane of the wave decodes the same bits.  What is read from memory then goes through the first lane, which tells the
  // compiler that the whole decoder state is one value per wave: it is kept in scalar registers and stepped by the scalar unit
  bool wave_uniform;
  PF_PNGD_HD Bits(const uint32_t* words, uint32_t bits, bool uniform_in_wave = false) : w(words), nbits(bits), wave_uniform(uniform_in_wave) {}
};

PF_PNGD_HD uint32_t uniform(const Bits& b, uint32_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
  if (b.wave_uniform) return (uint32_t)__builtin_amdgcn_readfirstlane((int)x);
#endif
  (void)b;
  return x;
}

PF_PNGD_HD uint32_t peek(Bits& b, uint32_t p) {      // the 32 bits at p, first bit lowest
  if (p >= b.nbits) return 0;
  const uint32_t i = p >> 5;
  if (i != b.wi) {
    b.lo = i == b.wi + 1 ? b.hi : uniform(b, b.w[i]);
    b.hi = uniform(b, b.w[i + 1]);
    b.wi = i;
  }
  const uint64_t v = ((uint64_t)b.hi << 32) | b.lo;
  return (uint32_t)(v >> (p & 31u));
}

struct Code {
  uint16_t* count;        // [16] symbols per length
  uint16_t* symbol;       // symbols in canonical order
  uint16_t* fast;         // [1 << fast_bits] by the next bits of the stream: length << 9 | symbol, 0 = a longer code or none; may be null
  int fast_bits;
};
constexpr int LIT_FAST_BITS = 10, DIST_FAST_BITS = 8, CL_FAST_BITS = 0;

PF_PNGD_HD uint32_t reverse_bits(uint32_t v, int n) {
  uint32_t r = 0;
  for (int i = 0; i < n; ++i) r |= ((v >> i) & 1u) << (n - 1 - i);
  return r;
}

// count / symbol of the code with lengths len[0..n); offs: 16 words of scratch.  -> Kraft sum in units of 2^-15 (1 << 15 = complete)
PF_PNGD_HD uint32_t build_code(const Code& c, const uint8_t* len, int n, uint16_t* offs) {
  for (int l = 0; l < 16; ++l) c.count[l] = 0;
  for (int s = 0; s < n; ++s) c.count[len[s] & 15]++;
  uint32_t kraft = 0;
  offs[1] = 0;
  for (int l = 1; l < 16; ++l) {
    kraft += (uint32_t)c.count[l] << (15 - l);
    if (l < 15) offs[l + 1] = offs[l] + c.count[l];
  }
  for (int s = 0; s < n; ++s)
    if (len[s] & 15) c.symbol[offs[len[s] & 15]++] = (uint16_t)s;
  if (c.fast && kraft <= (1u << 15)) {          // every code of at most fast_bits bits, at each table place that begins with it
    const uint32_t size = 1u << c.fast_bits;
    for (uint32_t j = 0; j < size; ++j) c.fast[j] = 0;
    uint32_t code = 0, index = 0;
    for (int l = 1; l <= c.fast_bits; ++l) {
      code <<= 1;
      for (uint32_t k = 0; k < c.count[l]; ++k, ++code, ++index) {
        const uint16_t e = (uint16_t)((l << 9) | c.symbol[index]);
        for (uint32_t j = reverse_bits(code, l); j < size; j += 1u << l) c.fast[j] = e;
      }
    }
  }
  return kraft;
}

// literal/length code: complete or one 1-bit code; distance code: complete, one 1-bit code or empty (zlib's and puff's rule)
PF_PNGD_HD bool lit_kraft_ok(uint32_t kraft, uint32_t nonzero) { return kraft == (1u << 15) || (nonzero == 1 && kraft == (1u << 14)); }
PF_PNGD_HD bool dist_kraft_ok(uint32_t kraft, uint32_t nonzero) { return nonzero == 0 || lit_kraft_ok(kraft, nonzero); }

PF_PNGD_HD int decode_sym(Bits& b, uint32_t& p, const Code& c) {      // -> symbol, or -1 when no code matches (nothing consumed)
  uint32_t v = peek(b, p);
  if (c.fast) {
    const uint32_t e = uniform(b, c.fast[v & ((1u << c.fast_bits) - 1u)]);
    if (e) {
      p += e >> 9;
      return (int)(e & 511u);
    }
  }
  int code = 0, first = 0, index = 0;
  for (int len = 1; len <= 15; ++len) {
    code |= (int)(v & 1u);
    v >>= 1;
    const int count = (int)uniform(b, c.count[len]);
    if (code - count < first) {
      p += len;
      return (int)uniform(b, c.symbol[index + (code - first)]);
    }
    index += count;
    first = (first + count) << 1;
    code <<= 1;
  }
  return -1;
}

// the order in which a dynamic header sends the lengths of the code-length code, 5 bits each
constexpr uint64_t cl_order_word(int from) {
  const int order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
  uint64_t w = 0;
  for (int i = 0; i < 12 && from + i < 19; ++i) w |= (uint64_t)order[from + i] << (5 * i);
  return w;
}
constexpr uint64_t CL_ORDER_LO = cl_order_word(0), CL_ORDER_HI = cl_order_word(12);
PF_PNGD_HD int cl_order(int i) { return (int)(((i < 12 ? CL_ORDER_LO >> (5 * i) : CL_ORDER_HI >> (5 * (i - 12)))) & 31u); }

// The block finder's test: does a well-formed dynamic block header (BTYPE 10) start at p (the BFINAL bit)?  Keeps everything in
// registers: the 19 code-length-code lengths in one word, its canonical order in two, the two big codes only as running Kraft sums.
PF_PNGD_HD bool probe_dynamic(Bits& b, uint32_t p) {
  uint32_t v = peek(b, p);
  if (((v >> 1) & 3u) != 2u) return false;
  const int nlit = 257 + (int)((v >> 3) & 31u), ndist = 1 + (int)((v >> 8) & 31u), ncl = 4 + (int)((v >> 13) & 15u);
  if (nlit > 286 || ndist > 30) return false;
  p += 17;
  uint64_t cl = 0;                       // 3 bits per symbol
  uint32_t kraft = 0;
  for (int i = 0; i < ncl; ++i) {
    const uint32_t l = (peek(b, p) & 7u);
    p += 3;
    cl |= (uint64_t)l << (3 * cl_order(i));
    if (l) kraft += 128u >> l;
  }
  if (kraft != 128u) return false;
  uint64_t cnt = 0, sorted_lo = 0, sorted_hi = 0;     // 5 bits per length / per place
  int place = 0;
  for (int l = 1; l <= 7; ++l)
    for (int s = 0; s < 19; ++s)
      if ((int)((cl >> (3 * s)) & 7u) == l) {
        cnt += 1ull << (5 * l);
        if (place < 12) sorted_lo |= (uint64_t)s << (5 * place);
        else sorted_hi |= (uint64_t)s << (5 * (place - 12));
        ++place;
      }
  uint32_t kl = 0, kd = 0, nl = 0, nd = 0;
  bool has_end = false;
  int prev = 0;
  for (int i = 0; i < nlit + ndist;) {
    v = peek(b, p);
    int code = 0, first = 0, index = 0, sym = -1;
    for (int len = 1; len <= 7; ++len) {
      code |= (int)(v & 1u);
      v >>= 1;
      const int count = (int)((cnt >> (5 * len)) & 31u);
      if (code - count < first) {
        const int at = index + (code - first);
        sym = (int)((at < 12 ? sorted_lo >> (5 * at) : sorted_hi >> (5 * (at - 12))) & 31u);
        p += len;
        break;
      }
      index += count;
      first = (first + count) << 1;
      code <<= 1;
    }
    if (sym < 0) return false;
    int rep = 1, l = sym;
    if (sym == 16) {
      if (i == 0) return false;
      l = prev;
      rep = 3 + (int)(v & 3u);
      p += 2;
    } else if (sym == 17) {
      l = 0;
      rep = 3 + (int)(v & 7u);
      p += 3;
    } else if (sym == 18) {
      l = 0;
      rep = 11 + (int)(v & 127u);
      p += 7;
    }
    if (i + rep > nlit + ndist || p > b.nbits) return false;
    prev = l;
    for (int r = 0; r < rep; ++r, ++i) {
      if (!l) continue;
      if (i < nlit) { kl += 1u << (15 - l); ++nl; if (i == 256) has_end = true; }
      else { kd += 1u << (15 - l); ++nd; }
    }
  }
  return has_end && lit_kraft_ok(kl, nl) && dist_kraft_ok(kd, nd);
}

// Reads the header of a dynamic block (p just past BFINAL and BTYPE) into lens[0 .. nlit + ndist).  cl: count[16] and symbol[19] of
// scratch for the code-length code; offs: 16 words.  -> S_OK or S_INVALID
PF_PNGD_HD int read_dynamic_header(Bits& b, uint32_t& p, uint8_t* lens, int& nlit, int& ndist, const Code& cl, uint16_t* offs) {
  uint32_t v = peek(b, p);
  nlit = 257 + (int)(v & 31u);
  ndist = 1 + (int)((v >> 5) & 31u);
  const int ncl = 4 + (int)((v >> 10) & 15u);
  p += 14;
  if (nlit > 286 || ndist > 30) return S_INVALID;
  for (int i = 0; i < 19; ++i) lens[i] = 0;
  for (int i = 0; i < ncl; ++i) {
    lens[cl_order(i)] = (uint8_t)(peek(b, p) & 7u);
    p += 3;
  }
  if (build_code(cl, lens, 19, offs) != (1u << 15)) return S_INVALID;
  const int total = nlit + ndist;
  for (int i = 0; i < total;) {
    const int sym = decode_sym(b, p, cl);
    if (sym < 0) return S_INVALID;
    v = peek(b, p);
    int rep = 1, l = sym;
    if (sym == 16) {
      if (i == 0) return S_INVALID;
      l = lens[i - 1];
      rep = 3 + (int)(v & 3u);
      p += 2;
    } else if (sym == 17) {
      l = 0;
      rep = 3 + (int)(v & 7u);
      p += 3;
    } else if (sym == 18) {
      l = 0;
      rep = 11 + (int)(v & 127u);
      p += 7;
    }
    if (i + rep > total || p > b.nbits) return S_INVALID;
    for (int r = 0; r < rep; ++r) lens[i++] = (uint8_t)l;
  }
  return lens[256] ? S_OK : S_INVALID;
}

PF_PNGD_HD void fixed_lens(uint8_t* lens, int& nlit, int& ndist) {
  nlit = 288;
  ndist = 30;
  for (int i = 0; i < 288; ++i) lens[i] = (uint8_t)(i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : 8);
  for (int i = 0; i < 30; ++i) lens[288 + i] = 5;
}

// Header of the block at p (the BFINAL bit) of type 1 or 2 -> the two codes, p at the first symbol.  lens: MAX_LENS bytes; lit.symbol
// [288], dist.symbol [32] (also the scratch of the code-length code), offs [16], the fast tables 1 << LIT_FAST_BITS and 1 << DIST_FAST_BITS.  -> S_OK or S_INVALID
PF_PNGD_HD int read_block_codes(Bits& b, uint32_t& p, uint8_t* lens, const Code& lit, const Code& dist, uint16_t* offs) {
  const uint32_t type = (peek(b, p) >> 1) & 3u;
  p += 3;
  int nlit, ndist;
  if (type == 1) fixed_lens(lens, nlit, ndist);
  else if (type != 2 || read_dynamic_header(b, p, lens, nlit, ndist, Code{dist.count, dist.symbol, nullptr, 0}, offs) != S_OK) return S_INVALID;
  uint32_t nl = 0, nd = 0;
  for (int i = 0; i < nlit; ++i) nl += lens[i] != 0;
  for (int i = 0; i < ndist; ++i) nd += lens[nlit + i] != 0;
  if (type == 1) {                     // the fixed distance code is 30 of 32 five-bit codes: complete as sent, 30 and 31 never valid
    build_code(lit, lens, nlit, offs);
    build_code(dist, lens + nlit, ndist, offs);
    return S_OK;
  }
  if (!lit_kraft_ok(build_code(lit, lens, nlit, offs), nl)) return S_INVALID;
  if (!dist_kraft_ok(build_code(dist, lens + nlit, ndist, offs), nd)) return S_INVALID;
  return S_OK;
}

PF_PNGD_HD void length_code(int s, int& base, int& extra) {       // s = symbol - 257 in 0 .. 28
  if (s < 8) { base = 3 + s; extra = 0; }
  else if (s == 28) { base = 258; extra = 0; }
  else { extra = (s >> 2) - 1; base = 3 + ((4 + (s & 3)) << extra); }
}
PF_PNGD_HD void distance_code(int d, int& base, int& extra) {     // d in 0 .. 29
  if (d < 4) { base = 1 + d; extra = 0; }
  else { extra = (d >> 1) - 1; base = 1 + ((2 + (d & 1)) << extra); }
}

// The symbols of one block from p to its end-of-block code, at most up to bit `stop` (<= nbits).  The sink takes literal(byte) -> bool
// and match(length, distance) -> status.  -> S_OK with p behind the end-of-block code, or why it stopped
template <class Sink>
PF_PNGD_HD int decode_symbols(Bits& b, uint32_t& p, uint32_t stop, const Code& lit, const Code& dist, Sink& out) {
  while (p < stop) {
    int s = decode_sym(b, p, lit);
    if (s < 0) return S_INVALID;
    if (s < 256) {
      if (!out.literal((uint8_t)s)) return S_SIZE;
      continue;
    }
    if (s == 256) return p > b.nbits ? S_EOS : S_OK;
    s -= 257;
    if (s > 28) return S_INVALID;
    int base, extra;
    length_code(s, base, extra);
    const int len = base + (int)(peek(b, p) & ((1u << extra) - 1u));
    p += extra;
    const int d = decode_sym(b, p, dist);
    if (d < 0 || d > 29) return S_INVALID;
    distance_code(d, base, extra);
    const uint32_t back = (uint32_t)base + (peek(b, p) & ((1u << extra) - 1u));
    p += extra;
    if (p > b.nbits) return S_EOS;
    const int r = out.match((uint32_t)len, back);
    if (r != S_OK) return r;
  }
  return stop >= b.nbits ? S_EOS : S_LIMIT;
}

struct CountSink {        // the scan pass: counts, stores nothing
  uint32_t n, cap;
  PF_PNGD_HD bool literal(uint8_t) { return ++n <= cap; }
  PF_PNGD_HD int match(uint32_t len, uint32_t) { n += len; return n <= cap ? S_OK : S_SIZE; }
};

// The inflate pass: a literal goes to lit[o] with ref[o] = o; a matched byte gets the root of its source: ref[source] when the source
// lies in this block (already a literal's place or a place in an earlier block), the source itself otherwise.  [base, end) is the block.
struct RefSink {
  uint8_t* lit;
  uint32_t* ref;
  uint32_t o, base, end;
  PF_PNGD_HD bool literal(uint8_t v) {
    if (o >= end) return false;
    lit[o] = v;
    ref[o] = o;
    ++o;
    return true;
  }
  PF_PNGD_HD int match(uint32_t len, uint32_t back) {
    if (back > o) return S_DIST;
    if (len > end - o) return S_SIZE;
    for (uint32_t k = 0; k < len; ++k, ++o) {
      const uint32_t s = o - back;
      ref[o] = s >= base ? ref[s] : s;
    }
    return S_OK;
  }
};

PF_PNGD_HD uint32_t scan_stop(const Bits& b, uint32_t start, uint32_t max_bits) {
  return (start < b.nbits && b.nbits - start > max_bits) ? start + max_bits : b.nbits;
}

// scan record of one candidate: words {start bit, end bit, output bytes, status | BFINAL << 8}
PF_PNGD_HD void scan_block(Bits b, uint32_t start, uint32_t max_bits, uint32_t expected, uint8_t* lens, const Code& lit, const Code& dist,
                           uint16_t* offs, uint32_t* rec) {
  uint32_t p = start;
  const uint32_t bfinal = peek(b, p) & 1u;
  CountSink sink{0, expected};
  int st = start < b.nbits ? read_block_codes(b, p, lens, lit, dist, offs) : S_EOS;
  if (st == S_OK) st = decode_symbols(b, p, scan_stop(b, start, max_bits), lit, dist, sink);
  rec[0] = start;
  rec[1] = p;
  rec[2] = sink.n;
  rec[3] = (uint32_t)st | (bfinal << 8);
}

// ---- decoding inside a block in parallel subsequences (csrc/png_inflate_par.hip on the device, png_host.h on the host)
//
// The stream is cut into lanes, the absolute bit ranges [jS, (j + 1)S).  A lane decodes from an entry bit, taken to be the start of a
// literal/length code, the tokens that start in front of its end; its exit is the start of the first token at or behind the end, which
// is the next lane's true entry.  A block is worked through in windows of PAR_WINDOW lanes: lane 0 of a window starts from the known
// entry, every other lane first guesses its own jS, and in each round a lane whose predecessor's exit of the round before differs from
// its entry decodes again from that exit (a lane behind an end-of-block code is left as it is).  Lane k is final after round k, so the
// rounds of a window are at most PAR_WINDOW - 1 and end sooner when none changed.  Bounds: a lane turns only while p < end <= nbits and
// every turn consumes at least one bit (an invalid code exactly one), so a lane is bounded by end - entry.
#ifndef PF_PNGD_PAR_WINDOW
// lanes per window = threads per workgroup of the two kernels; the host models use the same number.  512 had the lowest whole-decode
// median on the two RGB level-6 files of profiles/png_inflate_par_time.json (5.11 + 16.35 ms against 4.93 + 16.68 ms with 1024 threads
// and 5.26 + 16.26 ms with 256)
#define PF_PNGD_PAR_WINDOW 512
#endif
constexpr int PAR_WINDOW = PF_PNGD_PAR_WINDOW;
constexpr uint32_t PAR_MIN_BITS = 64, PAR_MAX_BITS = 1u << 16;        // a lane's length: a multiple of 32 in this range

PF_PNGD_HD bool par_bits_ok(uint32_t s) { return s >= PAR_MIN_BITS && s <= PAR_MAX_BITS && (s & 31u) == 0; }

enum { L_EOB = 1, L_INVALID = 2 };
struct Lane {
  uint32_t exit;          // the start of the first token at or behind the lane's end (behind the end-of-block code when one was read)
  uint32_t bytes;         // output bytes of the lane's tokens: below 2^24 (at most 2^15 matches of 258 bytes in 2^16 bits)
  uint32_t eob;           // the bit behind the end-of-block code, when L_EOB is set
  uint32_t flags;         // L_EOB; L_INVALID: an invalid code, a length symbol above 285, a distance symbol above 29, or a token that
                          // runs past the end of the stream
  int sink;               // S_OK, or the status with which the sink refused a token (the lane ends there)
};

// The tokens that start in [p, end), end <= b.nbits.  A literal is one token; a length, its extra bits, the distance code and its extra
// bits are one token.  An invalid code consumes one bit and produces nothing; an end-of-block code ends the lane; p >= end produces
// nothing and passes p on.  The sink takes literal(byte) -> bool and match(length, distance) -> status, as in decode_symbols.
template <class Sink>
PF_PNGD_HD Lane decode_lane(Bits& b, uint32_t p, uint32_t end, const Code& lit, const Code& dist, Sink& out) {
  Lane r{p, 0u, 0u, 0u, S_OK};
  while (p < end) {
    const uint32_t token = p;
    int s = decode_sym(b, p, lit);
    if (s >= 0 && s < 256) {
      if (!out.literal((uint8_t)s)) { r.sink = S_SIZE; break; }
      ++r.bytes;
      continue;
    }
    if (s == 256) {
      r.flags |= L_EOB;
      r.eob = p;
      break;
    }
    s -= 257;
    if (s >= 0 && s <= 28) {
      int base, extra;
      length_code(s, base, extra);
      const int len = base + (int)(peek(b, p) & ((1u << extra) - 1u));
      p += extra;
      const int d = decode_sym(b, p, dist);
      if (d >= 0 && d <= 29) {
        distance_code(d, base, extra);
        const uint32_t back = (uint32_t)base + (peek(b, p) & ((1u << extra) - 1u));
        p += extra;
        if (p > b.nbits) { r.flags |= L_INVALID; break; }
        const int st = out.match((uint32_t)len, back);
        if (st != S_OK) { r.sink = st; break; }
        r.bytes += (uint32_t)len;
        continue;
      }
    }
    r.flags |= L_INVALID;
    p = token + 1;
  }
  r.exit = p;
  return r;
}

struct NullSink {         // the rounds: only the lane's exit and byte count matter
  PF_PNGD_HD bool literal(uint8_t) { return true; }
  PF_PNGD_HD int match(uint32_t, uint32_t) { return S_OK; }
};

// lane j of a stream cut every S bits, clipped to `stop`
PF_PNGD_HD uint32_t lane_end(uint32_t j, uint32_t S, uint32_t stop) {
  const uint64_t e = ((uint64_t)j + 1u) * S;
  return e < stop ? (uint32_t)e : stop;
}
// How many of the window's PAR_WINDOW places, from lane `first` (first * S < stop) on, are lanes: those that begin in front of `stop`.
// The places behind them hold nothing and take no part in the rounds.
PF_PNGD_HD int lanes_in_window(uint32_t first, uint32_t S, uint32_t stop) {
  const uint32_t n = (stop - 1u) / S + 1u - first;
  return n < (uint32_t)PAR_WINDOW ? (int)n : PAR_WINDOW;
}

// What the true chain of a window comes to: lanes 0, 1, ... up to the first that read an end-of-block code.  e, fi, fs: the first lane
// with L_EOB, with L_INVALID, and whose running output total exceeds `expected` (PAR_WINDOW when there is none).  -> the lane at which
// the block's decode ends (PAR_WINDOW: it goes on behind the window's last lane) and in `st` how: an invalid code counts in front of a size
// overflow in the same lane, and both in front of the end-of-block code.
PF_PNGD_HD int chain_event(int e, int fi, int fs, int& st) {
  st = S_OK;
  if (fi < PAR_WINDOW && fi <= e && fi <= fs) { st = S_INVALID; return fi; }
  if (fs < PAR_WINDOW && fs <= e) { st = S_SIZE; return fs; }
  return e;
}

}  // namespace pf_pngd
