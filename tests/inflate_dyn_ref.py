"""A pure-Python restatement of the device inflate that decodes dynamic-Huffman blocks (csrc/inflate_dyn_core.h,
csrc/inflate_dyn.hip): the segment rule of tests/inflate_ref.py with one change - a BTYPE 10 block is decoded, not
refused - and the chain ``fnn_inflate_segments_dyn`` follows.  Test infrastructure only.

A table header is accepted exactly where zlib's inflate accepts it; every refusal of one is TABLES.  The checks are made in
the order of ``InfDynCodes::header``, the limit first behind every step, so that refusals agree reason for reason and byte
count for byte count:
  1. HLIT <= 286 and HDIST <= 30, behind the 14 bits of HLIT, HDIST and HCLEN;
  2. the code-length code is complete (neither over-subscribed nor incomplete nor empty);
  3. 16 at position 0, and a run that overshoots HLIT + HDIST (the lengths are one sequence);
  4. the length of symbol 256 is not 0;
  5. the literal / length set, then the distance set: not over-subscribed, incomplete only with no code longer than 1 bit.
A bit pattern that belongs to no symbol of an accepted incomplete set takes 1 bit and is SYMBOL."""
import zlib

from inflate_ref import (BTYPE3, CHAIN, DISTANCE, DYNAMIC, END, FINAL, INPUT, INPUT_MAX, NLEN, OK, OUTPUT, SEGMENT_MAX, SIZE, SYMBOL,  # noqa: F401
                         _DIST_BASE, _DIST_EXTRA, _FIXED, _LEN_BASE, _LEN_EXTRA, _rev, candidates, full_flush_stream, inflate_raw,
                         label_runs, marker_ends, random_bytes, texty_bytes)
from inflate_ref import REASONS as _FIXED_REASONS

TABLES = 12
REASONS = _FIXED_REASONS + ('TABLES',)
ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)


def build_code(lens, may_be_short: bool):
    """The canonical code of the lengths -> {(bits, code, first bit highest): symbol}, or None where the set is refused: an
    over-subscribed one always, an incomplete one unless ``may_be_short`` and no code is longer than 1 bit."""
    count = [0] * 16
    for n in lens:
        count[n] += 1
    left, nxt, code = 1, [0] * 16, 0
    for bits in range(1, 16):
        left = 2 * left - count[bits]
        if left < 0:
            return None
        nxt[bits] = code
        code = (code + count[bits]) << 1
    if left > 0 and not (may_be_short and max(lens, default=0) <= 1):
        return None
    table = {}
    for sym, n in enumerate(lens):
        if n:
            table[n, nxt[n]] = sym
            nxt[n] += 1
    return table


def decode_segment(data: bytes, start: int):
    """The segment of ``data`` that starts at byte ``start`` -> ``(end, out, reason)``, as ``inflate_ref.decode_segment``."""
    data = bytes(data)
    p = 8 * start
    end_bit, budget_bit = 8 * len(data), 8 * (start + INPUT_MAX)
    limit = min(end_bit, budget_bit)
    out = bytearray()

    def take(k):
        nonlocal p
        v = (int.from_bytes(data[p >> 3:(p >> 3) + 8], 'little') >> (p & 7)) & ((1 << k) - 1)
        p += k
        return v

    def stop(reason):
        return -1, bytes(out), reason

    def over():
        return END if p > end_bit else INPUT

    def symbol(table):
        """The next symbol of a canonical code; a pattern that belongs to none: 1 bit and -1."""
        nonlocal p
        v = take(15)
        p -= 15
        code = 0
        for n in range(1, 16):
            code = code << 1 | (v >> (n - 1) & 1)
            if (n, code) in table:
                p += n
                return table[n, code]
        p += 1
        return -1

    def tables():
        """The table header behind BTYPE 10 -> ``(literal / length code, distance code)`` or the reason."""
        hlit, hdist, hclen = 257 + take(5), 1 + take(5), 4 + take(4)
        if p > limit:
            return over()
        if hlit > 286 or hdist > 30:
            return TABLES
        cl = [0] * 19
        for i in range(hclen):
            cl[ORDER[i]] = take(3)
            if p > limit:
                return over()
        cl_code = build_code(cl, False)
        if cl_code is None:
            return TABLES
        lens = []
        while len(lens) < hlit + hdist:
            sym = symbol(cl_code)
            rep, n = 1, sym
            if sym == 16:
                rep, n = 3 + take(2), lens[-1] if lens else 0
            elif sym == 17:
                rep, n = 3 + take(3), 0
            elif sym == 18:
                rep, n = 11 + take(7), 0
            if p > limit:
                return over()
            if sym < 0 or (sym == 16 and not lens) or len(lens) + rep > hlit + hdist:
                return TABLES
            lens += [n] * rep
        if lens[256] == 0:
            return TABLES
        lit = build_code(lens[:hlit], True)
        if lit is None:
            return TABLES
        dist = build_code(lens[hlit:], True)
        if dist is None:
            return TABLES
        return lit, dist

    while True:
        hdr = take(3)
        if p > limit:
            return stop(over())
        if hdr & 1:
            return stop(FINAL)
        if hdr >> 1 == 3:
            return stop(BTYPE3)
        if hdr >> 1 == 0:
            p += -p & 7
            n, nn = take(16), take(16)
            if p > limit:
                return stop(over())
            if n ^ nn != 0xFFFF:
                return stop(NLEN)
            if n == 0:
                return p >> 3, bytes(out), OK
            if len(out) + n > SEGMENT_MAX:
                return stop(OUTPUT)
            if p + 8 * n > limit:
                return stop(END if p + 8 * n > end_bit else INPUT)
            out += data[p >> 3:(p >> 3) + n]
            p += 8 * n
            continue
        codes = None
        if hdr >> 1 == 2:
            codes = tables()
            if isinstance(codes, int):
                return stop(codes)
        while True:
            if codes is None:
                sym, n = _FIXED[take(9)]
                p -= 9 - n
            else:
                sym = symbol(codes[0])
            if p > limit:
                return stop(over())
            if 0 <= sym < 256:
                if len(out) >= SEGMENT_MAX:
                    return stop(OUTPUT)
                out.append(sym)
                continue
            if sym == 256:
                break
            if sym < 0 or sym > 285:
                return stop(SYMBOL)
            length = _LEN_BASE[sym - 257] + take(_LEN_EXTRA[sym - 257])
            code = _rev(take(5), 5) if codes is None else symbol(codes[1])
            if code < 0 or code > 29:
                return stop(SYMBOL)
            dist = _DIST_BASE[code] + take(_DIST_EXTRA[code])
            if p > limit:
                return stop(over())
            if dist > len(out):
                return stop(DISTANCE)
            if len(out) + length > SEGMENT_MAX:
                return stop(OUTPUT)
            for _ in range(length):
                out.append(out[-dist])


def chain(stream: bytes, starts, out_bytes: int):
    """What ``fnn_inflate_segments_dyn`` reports -> ``(status, bytes or None, crc32)``: ``inflate_ref.chain`` with this rule."""
    stream = bytes(stream)
    starts = list(starts)
    if not starts or not stream:
        return (OK if out_bytes == 0 else SIZE), (b'' if out_bytes == 0 else None), 0
    assert starts[0] == 0 and all(a < b for a, b in zip(starts, starts[1:])) and starts[-1] < len(stream)
    known = set(starts)
    at, pieces, total = 0, [], 0
    while True:
        end, out, reason = decode_segment(stream, at)
        if reason != OK:
            return reason, None, 0
        pieces.append(out)
        total += len(out)
        if total > out_bytes:
            return SIZE, None, 0
        if end == len(stream):
            break
        if end not in known:
            return CHAIN, None, 0
        at = end
    if total != out_bytes:
        return SIZE, None, 0
    made = b''.join(pieces)
    return OK, made, zlib.crc32(made)
