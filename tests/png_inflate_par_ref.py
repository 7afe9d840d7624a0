"""Slow, plain model of the subsequence decode of csrc/png_inflate.h / csrc/png_inflate_par.hip, on the Bits, read_codes and tables of
tests/png_decode_ref.py: the lane decoder, the rounds of a window and the record a candidate comes to.  It states the scheme a second
time, independently of the C code, so that the C host model's round counts and records can be held against it."""
from tests import png_decode_ref as R


def decode_lane(b, p, end, lit, dist):
    """the tokens that start in [p, end) -> (exit bit, output bytes, bit behind the end-of-block code or None, invalid code met)"""
    n, eob, invalid = 0, None, False
    while p < end:
        token = p
        e = lit[b.peek(p, 15)]
        if e >= 0:
            p += e >> 9
            s = e & 511
            if s < 256:
                n += 1
                continue
            if s == 256:
                eob = p
                break
            s -= 257
            if s <= 28:
                length = R.LEN_BASE[s] + b.peek(p, R.LEN_EXTRA[s])
                p += R.LEN_EXTRA[s]
                e = dist[b.peek(p, 15)]
                if e >= 0 and (e & 511) <= 29:
                    p += (e >> 9) + R.DIST_EXTRA[e & 511]
                    if p > b.nbits:                   # the token runs past the stream
                        invalid = True
                        break
                    n += length
                    continue
        invalid = True                                # consumes one bit, produces nothing
        p = token + 1
    return p, n, eob, invalid


def window_rounds(b, first, carry, stop, S, T, lit, dist):
    """the lanes of the window that begins with lane `first` (at most T), lane 0 entering at carry -> (entries, lanes, rounds in which a lane changed)"""
    live = min(T, (stop - 1) // S + 1 - first)        # the window's places that begin in front of stop: only these are lanes
    ends = [min((first + k + 1) * S, stop) for k in range(live)]
    entry = [carry if k == 0 else (first + k) * S for k in range(live)]
    lane = [decode_lane(b, entry[k], ends[k], lit, dist) for k in range(live)]
    rounds = 0
    for r in range(1, live):
        prev, changed = list(lane), False             # a round reads only the round before
        for k in range(1, live):
            if prev[k - 1][2] is not None or prev[k - 1][0] == entry[k]:
                continue
            entry[k] = prev[k - 1][0]
            lane[k] = decode_lane(b, entry[k], ends[k], lit, dist)
            changed = True
        if not changed:
            break
        rounds = r
    return entry, lane, rounds


def scan(b, start, max_bits, expected, S, T):
    """one candidate -> (start, end bit, output bytes, status, BFINAL, largest round count of its windows)"""
    final = b.peek(start, 1)
    codes = R.read_codes(b, start) if start < b.nbits else None
    if codes is None:
        return start, start, 0, R.S_INVALID, final, 0
    lit, dist, p = codes
    stop = min(start + max_bits, b.nbits)
    total, most, first = 0, 0, p // S
    while first * S < stop:
        _, lane, rounds = window_rounds(b, first, p, stop, S, T, lit, dist)
        most = max(most, rounds)
        for ex, n, eob, invalid in lane:              # the true chain, lane by lane
            total += n
            if invalid:
                return start, ex, total, R.S_INVALID, final, most
            if total > expected:
                return start, ex, total, R.S_SIZE, final, most
            if eob is not None:
                return start, eob, total, (R.S_EOS if eob > b.nbits else R.S_OK), final, most
        p = lane[-1][0]
        first += T
    return start, p, total, (R.S_EOS if stop >= b.nbits else R.S_LIMIT), final, most


def rounds_of_true_blocks(deflate, expected, S, T):
    """the true fixed and dynamic blocks of a stream (the chain of png_decode_ref.model) -> (their records from scan(), the largest round
    count among them)"""
    b = R.Bits(deflate)
    blocks = [k for k in R.model(deflate, expected)["blocks"] if k[1] != 0]
    recs = [scan(b, k[0], 1 << 21, expected, S, T) for k in blocks]
    return recs, max([r[5] for r in recs], default=0)
