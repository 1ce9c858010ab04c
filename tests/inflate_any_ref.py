"""A pure-Python restatement of the speculative device inflate (csrc/inflate_any_core.h, csrc/inflate_any.hip): the block
finder, the member rule with its reasons, the chain ``fnn_inflate_stream`` follows on the host, and the 16-bit entries with
their markers, the windows and the resolved bytes.  Test infrastructure only.

A candidate is bit 0, or a bit position where BFINAL 0, BTYPE 10 stand in front of a table header that
``inflate_dyn_ref``'s rule accepts and that ends inside the input.  A member is the decode from a candidate until a
non-final block ends at a candidate or a final block ends at the input's last byte."""
import zlib

import numpy as np

from inflate_dyn_ref import (BTYPE3, DISTANCE, END, FINAL, NLEN, OK, OUTPUT, REASONS, SIZE, SYMBOL, TABLES, ORDER,  # noqa: F401
                             _DIST_BASE, _DIST_EXTRA, _FIXED, _LEN_BASE, _LEN_EXTRA, _rev, build_code)

WINDOW = 32768
MARK = 0x8000


class _Bits:
    """The stream from bit ``p`` on; bits past the end of ``data`` read as 0."""

    def __init__(self, data: bytes, p: int):
        self.data, self.p, self.end = data, p, 8 * len(data)

    def take(self, k):
        p = self.p
        v = (int.from_bytes(self.data[p >> 3:(p >> 3) + 8], 'little') >> (p & 7)) & ((1 << k) - 1)
        self.p += k
        return v

    def symbol(self, table):
        v = self.take(15)
        self.p -= 15
        code = 0
        for n in range(1, 16):
            code = code << 1 | (v >> (n - 1) & 1)
            if (n, code) in table:
                self.p += n
                return table[n, code]
        self.p += 1
        return -1


def _tables(b: _Bits):
    """The table header at ``b`` -> ``(literal / length code, distance code)`` or the reason, in the order of
    ``InfDynCodes::header`` with the input's end as the limit."""
    hlit, hdist, hclen = 257 + b.take(5), 1 + b.take(5), 4 + b.take(4)
    if b.p > b.end:
        return END
    if hlit > 286 or hdist > 30:
        return TABLES
    cl = [0] * 19
    for i in range(hclen):
        cl[ORDER[i]] = b.take(3)
        if b.p > b.end:
            return END
    cl_code = build_code(cl, False)
    if cl_code is None:
        return TABLES
    lens = []
    while len(lens) < hlit + hdist:
        sym = b.symbol(cl_code)
        rep, n = 1, sym
        if sym == 16:
            rep, n = 3 + b.take(2), lens[-1] if lens else 0
        elif sym == 17:
            rep, n = 3 + b.take(3), 0
        elif sym == 18:
            rep, n = 11 + b.take(7), 0
        if b.p > b.end:
            return END
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


def is_candidate(data: bytes, p: int) -> bool:
    """The full rule at bit ``p``."""
    if p == 0:
        return len(data) > 0
    b = _Bits(data, p)
    if b.take(3) != 4 or b.p > b.end:
        return False
    return not isinstance(_tables(b), int)


def maybe(data: bytes):
    """The bit positions that pass the cheap first test (``inf_any_maybe``), ascending, as a numpy array: the three bits, HLIT
    and HDIST fields <= 29, the code-length code's Kraft sum exactly 1."""
    if not data:
        return np.zeros(0, np.int64)
    bits = np.unpackbits(np.frombuffer(bytes(data) + bytes(16), np.uint8), bitorder='little')
    n = 8 * len(data)
    p = np.flatnonzero((bits[0:n] == 0) & (bits[1:n + 1] == 0) & (bits[2:n + 2] == 1))

    def field(off, k):
        v = np.zeros(p.size, np.int64)
        for i in range(k):
            v |= bits[p + off + i].astype(np.int64) << i
        return v
    ok = (field(3, 5) <= 29) & (field(8, 5) <= 29)
    p = p[ok]
    hclen = 4 + field(13, 4)
    kraft = np.zeros(p.size, np.int64)
    for i in range(19):
        ln = field(17 + 3 * i, 3)
        kraft += np.where((i < hclen) & (ln > 0), 128 >> ln, 0)
    return p[kraft == 128]


def find(data: bytes):
    """All candidates of ``data`` in ascending order."""
    data = bytes(data)
    if not data:
        return []
    return [0] + [int(p) for p in maybe(data) if p and is_candidate(data, int(p))]


def find_slowly(data: bytes):
    """``find`` without the first test: the full rule at every bit."""
    data = bytes(data)
    return [p for p in range(8 * len(data)) if is_candidate(data, p)]


def decode_member(data: bytes, start: int, out_bytes: int, known):
    """The member of ``data`` that starts at bit ``start`` -> ``(end, entries, reason, reach)``: the bit behind it
    (8 * len(data): the stream's end; -1 when refused), its 16-bit entries (until the refusal), OK or why it stopped and how
    far before its own first byte it reaches.  ``known``: the set of candidates."""
    data = bytes(data)
    b = _Bits(data, start)
    out, reach = [], 0

    def stop(reason):
        return -1, out, reason, reach

    while True:
        hdr = b.take(3)
        if b.p > b.end:
            return stop(END)
        if hdr >> 1 == 3:
            return stop(BTYPE3)
        if hdr >> 1 == 0:
            b.p += -b.p & 7
            n, nn = b.take(16), b.take(16)
            if b.p > b.end:
                return stop(END)
            if n ^ nn != 0xFFFF:
                return stop(NLEN)
            if len(out) + n > out_bytes:
                return stop(OUTPUT)
            if b.p + 8 * n > b.end:
                return stop(END)
            out += data[b.p >> 3:(b.p >> 3) + n]
            b.p += 8 * n
        else:
            codes = None
            if hdr >> 1 == 2:
                codes = _tables(b)
                if isinstance(codes, int):
                    return stop(codes)
            while True:
                if codes is None:
                    sym, n = _FIXED[b.take(9)]
                    b.p -= 9 - n
                else:
                    sym = b.symbol(codes[0])
                if b.p > b.end:
                    return stop(END)
                if 0 <= sym < 256:
                    if len(out) >= out_bytes:
                        return stop(OUTPUT)
                    out.append(sym)
                    continue
                if sym == 256:
                    break
                if sym < 0 or sym > 285:
                    return stop(SYMBOL)
                length = _LEN_BASE[sym - 257] + b.take(_LEN_EXTRA[sym - 257])
                code = _rev(b.take(5), 5) if codes is None else b.symbol(codes[1])
                if code < 0 or code > 29:
                    return stop(SYMBOL)
                dist = _DIST_BASE[code] + b.take(_DIST_EXTRA[code])
                if b.p > b.end:
                    return stop(END)
                if len(out) + length > out_bytes:
                    return stop(OUTPUT)
                reach = max(reach, dist - len(out))
                for _ in range(length):
                    src = len(out) - dist
                    out.append(out[src] if src >= 0 else MARK | (WINDOW + src))
        if hdr & 1:
            if (b.p + 7) >> 3 != len(data):
                return stop(FINAL)
            return 8 * len(data), out, OK, reach
        if b.p in known:
            return b.p, out, OK, reach


def resolve(entries, window: bytes) -> bytes:
    """The entries with every marker replaced from the 32768 bytes that precede the member."""
    return bytes(e if e < MARK else window[e & (MARK - 1)] for e in entries)


class Result:
    """What ``fnn_inflate_stream`` does with a stream: ``status``; with OK also ``data`` and ``crc``; and the records of the
    passes as far as they went: ``candidates``, ``members`` as (start bit, offset, end, entries, reason, reach) and
    ``windows`` (window k precedes member k + 1)."""

    def __init__(self):
        self.status, self.data, self.crc, self.candidates, self.members, self.windows = OK, None, 0, [], [], []


def inflate(stream: bytes, out_bytes: int) -> Result:
    stream = bytes(stream)
    r = Result()
    if not stream:
        r.status = OK if out_bytes == 0 else SIZE
        r.data = b'' if out_bytes == 0 else None
        return r
    r.candidates = find(stream)
    known = set(r.candidates)
    at, off = 0, 0
    while True:
        end, entries, reason, reach = decode_member(stream, at, out_bytes, known)
        r.members.append((at, off, end, entries, reason, reach))
        if reason != OK:
            r.status = reason
            return r
        if reach > off:
            r.status = DISTANCE
            return r
        off += len(entries)
        if off > out_bytes:
            r.status = SIZE
            return r
        if end == 8 * len(stream):
            break
        at = end
    if off != out_bytes:
        r.status = SIZE
        return r
    window, pieces = bytes(WINDOW), []
    for m in r.members:
        piece = resolve(m[3], window)
        pieces.append(piece)
        window = (window + piece)[-WINDOW:]
        r.windows.append(window)
    r.windows.pop()
    r.data = b''.join(pieces)
    r.crc = zlib.crc32(r.data)
    return r


def dynamic_block_starts(stream: bytes):
    """A walk of a valid stream block by block from bit 0, without the candidate set: each block's start is where the one
    before it ended -> the bit position of every non-final dynamic block's header."""
    stream = bytes(stream)
    starts, b = [], _Bits(stream, 0)
    while True:
        at = b.p
        end, _, reason, _ = _one_block(stream, b)
        assert reason == OK, REASONS[reason]
        if end[1] == 2 and not end[0]:
            starts.append(at)
        if end[0]:
            return starts


def _one_block(stream, b):
    """Decodes exactly one block at ``b`` (no output kept) -> ((final, btype), None, reason, None)."""
    hdr = b.take(3)
    final, btype = hdr & 1, hdr >> 1
    if btype == 0:
        b.p += -b.p & 7
        n, nn = b.take(16), b.take(16)
        assert n ^ nn == 0xFFFF
        b.p += 8 * n
        return (final, btype), None, OK, None
    assert btype != 3
    codes = _tables(b) if btype == 2 else None
    assert not isinstance(codes, int)
    while True:
        if codes is None:
            sym, n = _FIXED[b.take(9)]
            b.p -= 9 - n
        else:
            sym = b.symbol(codes[0])
        if sym < 256:
            continue
        if sym == 256:
            return (final, btype), None, OK, None
        b.take(_LEN_EXTRA[sym - 257])
        code = _rev(b.take(5), 5) if codes is None else b.symbol(codes[1])
        b.take(_DIST_EXTRA[code])
