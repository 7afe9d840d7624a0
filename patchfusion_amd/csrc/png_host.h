// Host side of the PNG decoder (csrc/png_decode.hip): the chunk parser, the checksums, and a sequential restatement of the device
// algorithm (finder, scan records, chain walk, references, pointer jumping) over the code of png_inflate.h.  Like jpeg_host.h this header
// makes no GPU call and includes no GPU header, so a stand-alone program can include it (tests/host/png_decode_main.cpp runs it under the
// host sanitizers).
#pragma once
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../include/pf_hip.h"   // struct pf_pngd_header and the PF_PNGD_E_* codes: plain C declarations, no GPU header
#include "png_inflate.h"

namespace pf_pngd {

inline uint32_t rd32(const uint8_t* p) { return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3]; }

inline uint32_t crc32_update(uint32_t c, const uint8_t* p, long n) {
  static uint32_t table[256];
  static bool made = false;
  if (!made) {
    for (uint32_t i = 0; i < 256; ++i) {
      uint32_t v = i;
      for (int k = 0; k < 8; ++k) v = (v & 1u) ? 0xedb88320u ^ (v >> 1) : v >> 1;
      table[i] = v;
    }
    made = true;
  }
  for (long i = 0; i < n; ++i) c = table[(c ^ p[i]) & 255u] ^ (c >> 8);
  return c;
}

inline uint32_t adler32(const uint8_t* p, long n) {
  uint32_t a = 1, b = 0;
  for (long i = 0; i < n; ++i) {
    a = (a + p[i]) % 65521u;
    b = (b + a) % 65521u;
  }
  return (b << 16) | a;
}

inline int channels_of(int color_type) { return color_type == 0 || color_type == 3 ? 1 : color_type == 2 ? 3 : color_type == 4 ? 2 : 4; }

// Walks the chunks of a PNG file.  IHDR, PLTE and tRNS are validated, the IDAT payloads are concatenated behind their two-byte zlib
// header into deflate[0 .. *deflate_len) (capacity >= len is always enough) and that header is checked; ancillary chunks are skipped.
// The CRC of every critical chunk other than IDAT is checked, IDAT's only with check_idat_crc.
inline int parse(const uint8_t* d, long n, int check_idat_crc, pf_pngd_header* h, uint8_t* deflate, long capacity, long* deflate_len) {
  static const uint8_t SIG[8] = {137, 80, 78, 71, 13, 10, 26, 10};
  if (!d || !h || !deflate || !deflate_len) return 1;
  memset(h, 0, sizeof(*h));
  *deflate_len = 0;
  if (n < 8 || memcmp(d, SIG, 8)) return PF_PNGD_E_SIGNATURE;
  long at = 8, got = 0;
  bool seen_ihdr = false, seen_plte = false, seen_idat = false, idat_over = false, seen_iend = false;
  int zhead[2] = {0, 0}, nz = 0;
  while (!seen_iend) {
    if (n - at < 12) return PF_PNGD_E_CHUNK;
    const uint32_t len = rd32(d + at);
    const uint8_t* type = d + at + 4;
    if (len > 0x7fffffffu || (long)len > n - at - 12) return PF_PNGD_E_CHUNK;
    const uint8_t* body = type + 4;
    const bool is_idat = !memcmp(type, "IDAT", 4), critical = !(type[0] & 32u);
    if (!seen_ihdr && memcmp(type, "IHDR", 4)) return PF_PNGD_E_ORDER;
    if (critical && (!is_idat || check_idat_crc) && (crc32_update(0xffffffffu, type, 4 + (long)len) ^ 0xffffffffu) != rd32(body + len))
      return is_idat ? PF_PNGD_E_IDAT_CRC : PF_PNGD_E_CRC;
    if (!memcmp(type, "IHDR", 4)) {
      if (seen_ihdr) return PF_PNGD_E_ORDER;
      if (len != 13) return PF_PNGD_E_CHUNK;
      seen_ihdr = true;
      const uint32_t w = rd32(body), ht = rd32(body + 4);
      const int depth = body[8], ct = body[9];
      if (w == 0 || ht == 0 || w > 0x7fffffffu || ht > 0x7fffffffu || body[10] != 0 || body[11] != 0 || body[12] > 1) return PF_PNGD_E_IHDR;
      const bool ok = (ct == 0 && (depth == 1 || depth == 2 || depth == 4 || depth == 8 || depth == 16)) ||
                      (ct == 3 && (depth == 1 || depth == 2 || depth == 4 || depth == 8)) ||
                      ((ct == 2 || ct == 4 || ct == 6) && (depth == 8 || depth == 16));
      if (!ok) return PF_PNGD_E_IHDR;
      h->width = (int32_t)w; h->height = (int32_t)ht; h->depth = depth; h->color_type = ct; h->interlace = body[12];
      h->channels = channels_of(ct);
      const int bits = h->channels * depth;
      h->bpp = bits < 8 ? 1 : bits / 8;
      h->rowbytes = ((int64_t)w * bits + 7) / 8;
      h->inflated_bytes = (int64_t)ht * (1 + h->rowbytes);
      if (h->interlace) return PF_PNGD_E_INTERLACED;
    } else if (!memcmp(type, "PLTE", 4)) {
      if (seen_plte || seen_idat || len == 0 || len % 3 || len > 768) return seen_plte || seen_idat ? PF_PNGD_E_ORDER : PF_PNGD_E_PLTE;
      if (h->color_type == 0 || h->color_type == 4) return PF_PNGD_E_PLTE;
      if (h->color_type == 3 && (int)len / 3 > (1 << h->depth)) return PF_PNGD_E_PLTE;
      seen_plte = true;
      h->plte_entries = (int32_t)len / 3;
      memcpy(h->palette, body, len);
    } else if (is_idat) {
      if (idat_over) return PF_PNGD_E_ORDER;
      if (h->color_type == 3 && !seen_plte) return PF_PNGD_E_PLTE;
      seen_idat = true;
      h->idat_chunks++;
      h->compressed_bytes += len;
      long k = 0;
      for (; k < (long)len && nz < 2; ++k) zhead[nz++] = body[k];
      if (got + ((long)len - k) > capacity) return 1;
      memcpy(deflate + got, body + k, (size_t)((long)len - k));
      got += (long)len - k;
    } else if (!memcmp(type, "IEND", 4)) {
      seen_iend = true;
    } else if (critical) {
      return PF_PNGD_E_CHUNK;          // an unknown critical chunk
    } else if (!memcmp(type, "tRNS", 4)) {
      if (seen_idat || (h->color_type == 3 && !seen_plte)) return PF_PNGD_E_ORDER;
      const long want = h->color_type == 0 ? 2 : h->color_type == 2 ? 6 : -1;
      if (h->color_type == 4 || h->color_type == 6 || (want > 0 && (long)len != want) || (h->color_type == 3 && (int)len > h->plte_entries))
        return PF_PNGD_E_CHUNK;
      h->has_trns = 1;
    }
    if (seen_idat && !is_idat) idat_over = true;
    at += 12 + (long)len;
  }
  if (!seen_idat) return PF_PNGD_E_ORDER;
  if (nz < 2) return PF_PNGD_E_ZLIB;
  // CM = 8, window <= 32 KiB, no preset dictionary, FCHECK
  if ((zhead[0] & 15) != 8 || (zhead[0] >> 4) > 7 || (zhead[1] & 32) || ((zhead[0] << 8) | zhead[1]) % 31) return PF_PNGD_E_ZLIB;
  *deflate_len = got;
  return 0;
}

struct HostCodes {
  uint8_t lens[MAX_LENS];
  uint16_t lcount[16], lsymbol[288], dcount[16], dsymbol[32], offs[16], lfast[1 << LIT_FAST_BITS], dfast[1 << DIST_FAST_BITS];
  Code lit() { return Code{lcount, lsymbol, lfast, LIT_FAST_BITS}; }
  Code dist() { return Code{dcount, dsymbol, dfast, DIST_FAST_BITS}; }
};

// the deflate bytes as the padded words Bits wants
inline std::vector<uint32_t> pad_words(const uint8_t* deflate, long n) {
  std::vector<uint32_t> w((size_t)(n + 3) / 4 + PAD_WORDS, 0u);
  if (n > 0) memcpy(w.data(), deflate, (size_t)n);
  return w;
}

// The device algorithm, one step after the other: finder at every bit, a scan record per candidate, the chain walk (a fixed block that
// was not scanned is scanned when the walk reaches it), references, jumps, gather.  out: `expected` bytes.  -> 0, or a PF_PNGD_E_* code;
// stats: {dynamic, fixed, stored blocks, candidates, jump rounds that changed something, end byte of the deflate data}
inline int inflate_model(const uint8_t* deflate, long n, long expected, uint32_t max_block_bits, uint8_t* out, long* stats) {
  if (n <= 0 || n >= (1l << 28) || expected <= 0 || expected >= (1l << 31)) return PF_PNGD_E_STREAM;
  const std::vector<uint32_t> words = pad_words(deflate, n);
  Bits b(words.data(), (uint32_t)(8 * n));
  HostCodes hc;
  std::vector<uint32_t> recs;                       // four words per candidate, in stream order
  for (uint32_t p = 0; p < b.nbits; ++p) {
    const uint32_t type = (peek(b, p) >> 1) & 3u;
    if (!((p == 0 && type == 1) || (type == 2 && probe_dynamic(b, p)))) continue;
    uint32_t rec[4];
    scan_block(b, p, max_block_bits, (uint32_t)expected, hc.lens, hc.lit(), hc.dist(), hc.offs, rec);
    recs.insert(recs.end(), rec, rec + 4);
  }
  const long ncand = (long)recs.size() / 4;
  struct Block { uint32_t start, type, off, len; };
  std::vector<Block> blocks;
  uint32_t p = 0;
  long total = 0, count[3] = {0, 0, 0};
  for (;;) {
    if (p + 3 > b.nbits) return PF_PNGD_E_STREAM;
    const uint32_t head = peek(b, p), type = (head >> 1) & 3u;
    uint32_t rec[4] = {0, 0, 0, 0};
    if (type == 3) return PF_PNGD_E_STREAM;
    if (type == 0) {
      const long byte = ((long)p + 3 + 7) / 8;
      if (byte + 4 > n) return PF_PNGD_E_STREAM;
      const uint32_t len = deflate[byte] | (deflate[byte + 1] << 8), nlen = deflate[byte + 2] | (deflate[byte + 3] << 8);
      if ((len ^ nlen) != 0xffffu || byte + 4 + (long)len > n) return PF_PNGD_E_STREAM;
      blocks.push_back(Block{(uint32_t)(byte + 4), 0u, (uint32_t)total, len});
      total += len;
      p = (uint32_t)(8 * (byte + 4 + (long)len));
    } else {
      long lo = 0, hi = ncand;                      // the candidate that starts at p
      while (lo < hi) {
        const long mid = (lo + hi) / 2;
        if (recs[4 * (size_t)mid] < p) lo = mid + 1; else hi = mid;
      }
      if (lo < ncand && recs[4 * (size_t)lo] == p) memcpy(rec, &recs[4 * (size_t)lo], sizeof(rec));
      else if (type == 1) scan_block(b, p, max_block_bits, (uint32_t)expected, hc.lens, hc.lit(), hc.dist(), hc.offs, rec);
      else return PF_PNGD_E_STREAM;                 // a dynamic header the finder's test refuses is not a valid header
      if ((rec[3] & 255u) != S_OK) return (rec[3] & 255u) == S_SIZE ? PF_PNGD_E_SIZE : PF_PNGD_E_STREAM;
      blocks.push_back(Block{p, type, (uint32_t)total, rec[2]});
      total += rec[2];
      p = rec[1];
    }
    count[type == 2 ? 0 : type == 1 ? 1 : 2]++;
    if (total > expected) return PF_PNGD_E_SIZE;
    if (head & 1u) break;
  }
  if (total != expected) return PF_PNGD_E_SIZE;
  std::vector<uint8_t> lit((size_t)expected, 0);
  std::vector<uint32_t> ref((size_t)expected, 0u);
  for (const Block& k : blocks) {
    if (k.type == 0) {
      for (uint32_t i = 0; i < k.len; ++i) { lit[k.off + i] = deflate[k.start + i]; ref[k.off + i] = k.off + i; }
      continue;
    }
    uint32_t q = k.start;
    if (read_block_codes(b, q, hc.lens, hc.lit(), hc.dist(), hc.offs) != S_OK) return PF_PNGD_E_STREAM;
    RefSink sink{lit.data(), ref.data(), k.off, k.off, k.off + k.len};
    const int st = decode_symbols(b, q, b.nbits, hc.lit(), hc.dist(), sink);
    if (st == S_DIST) return PF_PNGD_E_DISTANCE;
    if (st != S_OK || sink.o != sink.end) return PF_PNGD_E_STREAM;
  }
  int rounds = 0;
  while ((1l << rounds) < (long)blocks.size()) ++rounds;
  ++rounds;
  long used = 0;
  for (int r = 0; r < rounds; ++r) {
    bool changed = false;
    for (long i = 0; i < expected; ++i) {
      const uint32_t a = ref[(size_t)i], c = ref[a];
      if (c != a) { ref[(size_t)i] = c; changed = true; }
    }
    if (changed) used = r + 1;
  }
  for (long i = 0; i < expected; ++i) {
    if (ref[ref[(size_t)i]] != ref[(size_t)i]) return PF_PNGD_E_STREAM;      // cannot happen: the fixed round count suffices
    out[i] = lit[ref[(size_t)i]];
  }
  if (stats) {
    stats[0] = count[0]; stats[1] = count[1]; stats[2] = count[2]; stats[3] = ncand; stats[4] = used; stats[5] = ((long)p + 7) / 8;
  }
  return 0;
}

// ---- the subsequence decode of csrc/png_inflate_par.hip in plain loops: the same lane decoder through the same round schedule
struct ParWindowHost {
  uint32_t entry[PAR_WINDOW];
  int live;               // the places of the window that are lanes
  Lane lane[PAR_WINDOW], prev[PAR_WINDOW];
};

// The rounds of the window whose first lane is `first` and whose lane 0 enters at `carry` -> the number of rounds in which a lane changed
inline uint32_t par_rounds(Bits& b, ParWindowHost& w, uint32_t first, uint32_t carry, uint32_t stop, uint32_t S, const Code& lit, const Code& dist) {
  NullSink null;
  const int live = w.live = lanes_in_window(first, S, stop);
  for (int k = 0; k < PAR_WINDOW; ++k) {
    w.entry[k] = k == 0 ? carry : (first + (uint32_t)k) * S;
    w.lane[k] = k < live ? decode_lane(b, w.entry[k], lane_end(first + (uint32_t)k, S, stop), lit, dist, null) : Lane{w.entry[k], 0u, 0u, 0u, S_OK};
  }
  uint32_t rounds = 0;
  for (int r = 1; r < live; ++r) {
    memcpy(w.prev, w.lane, sizeof(w.prev));           // a round reads only the round before
    bool changed = false;
    for (int k = 1; k < live; ++k) {
      if ((w.prev[k - 1].flags & L_EOB) || w.prev[k - 1].exit == w.entry[k]) continue;
      w.entry[k] = w.prev[k - 1].exit;
      w.lane[k] = decode_lane(b, w.entry[k], lane_end(first + (uint32_t)k, S, stop), lit, dist, null);
      changed = true;
    }
    if (!changed) break;
    rounds = (uint32_t)r;
  }
  return rounds;
}

// first lane with L_EOB, with L_INVALID, and whose running total (from `total`) exceeds `expected`
inline void par_firsts(const ParWindowHost& w, uint64_t total, uint64_t expected, int& e, int& fi, int& fs) {
  e = fi = fs = PAR_WINDOW;
  for (int k = 0; k < PAR_WINDOW; ++k) {
    total += w.lane[k].bytes;
    if (e == PAR_WINDOW && (w.lane[k].flags & L_EOB)) e = k;
    if (fi == PAR_WINDOW && (w.lane[k].flags & L_INVALID)) fi = k;
    if (fs == PAR_WINDOW && total > expected) fs = k;
  }
}

// scan_block with the symbols decoded in subsequences of S bits: the same record where scan_block's status is S_OK, some other status
// elsewhere.  -> the largest number of rounds a window needed
inline uint32_t scan_block_par(Bits b, uint32_t start, uint32_t max_bits, uint32_t expected, uint32_t S, HostCodes& hc, ParWindowHost& w, uint32_t* rec) {
  uint32_t p = start, rounds = 0;
  const uint32_t bfinal = peek(b, p) & 1u;
  uint64_t total = 0;
  int st = start < b.nbits ? read_block_codes(b, p, hc.lens, hc.lit(), hc.dist(), hc.offs) : S_EOS;
  if (st == S_OK) {
    const uint32_t stop = scan_stop(b, start, max_bits), j0 = p / S;
    st = stop >= b.nbits ? S_EOS : S_LIMIT;
    for (uint32_t first = j0; (uint64_t)first * S < stop; first += PAR_WINDOW) {
      const uint32_t r = par_rounds(b, w, first, p, stop, S, hc.lit(), hc.dist());
      if (r > rounds) rounds = r;
      int e, fi, fs, how;
      par_firsts(w, total, expected, e, fi, fs);
      const int at = chain_event(e, fi, fs, how);
      for (int k = 0; k < PAR_WINDOW && k <= at; ++k) total += w.lane[k].bytes;
      if (at < PAR_WINDOW) {
        const bool eob = how == S_OK;
        p = eob ? w.lane[at].eob : w.lane[at].exit;
        st = eob ? (p > b.nbits ? S_EOS : S_OK) : how;
        break;
      }
      p = w.lane[w.live - 1].exit;
    }
  }
  rec[0] = start;
  rec[1] = p;
  rec[2] = total > 0xffffffffull ? 0xffffffffu : (uint32_t)total;
  rec[3] = (uint32_t)st | (bfinal << 8);
  return rounds;
}

// The inflate pass of one fixed or dynamic block {start, type, offset, bytes}: the rounds, then every lane of the true chain decodes once
// more from its final entry into lit / ref, RefSink with `base` at the lane's own first output byte.  -> PF_PNGD_F_* flags
inline uint32_t inflate_block_par(Bits b, const uint32_t* blk, uint32_t S, HostCodes& hc, ParWindowHost& w, uint8_t* lit, uint32_t* ref, uint32_t* rounds) {
  uint32_t p = blk[0], flags = 0;
  const uint32_t off = blk[2], end = blk[2] + blk[3];
  if (read_block_codes(b, p, hc.lens, hc.lit(), hc.dist(), hc.offs) != S_OK) return PF_PNGD_F_STREAM;
  uint64_t total = 0;
  for (uint32_t first = p / S; (uint64_t)first * S < b.nbits; first += PAR_WINDOW) {
    const uint32_t r = par_rounds(b, w, first, p, b.nbits, S, hc.lit(), hc.dist());
    if (r > *rounds) *rounds = r;
    int e, fi, fs;
    par_firsts(w, 0, ~0ull, e, fi, fs);
    for (int k = 0; k < PAR_WINDOW && k <= e; ++k) {
      const uint64_t at = (uint64_t)off + total;
      const uint32_t o = at < end ? (uint32_t)at : end;
      RefSink sink{lit, ref, o, o, end};
      const Lane l = decode_lane(b, w.entry[k], lane_end(first + (uint32_t)k, S, b.nbits), hc.lit(), hc.dist(), sink);
      if (l.sink == S_DIST) flags |= PF_PNGD_F_DISTANCE;
      else if (l.sink != S_OK || (l.flags & L_INVALID)) flags |= PF_PNGD_F_STREAM;
      total += w.lane[k].bytes;
    }
    if (e < PAR_WINDOW) return (uint64_t)off + total == end ? flags : flags | PF_PNGD_F_STREAM;
    p = w.lane[w.live - 1].exit;
  }
  return flags | PF_PNGD_F_STREAM;            // the stream ended in front of the end-of-block code
}

}  // namespace pf_pngd
