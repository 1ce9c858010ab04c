"""A pure-Python restatement of the device inflate (csrc/inflate_core.h, csrc/inflate.hip): the segment rule with its
reasons, the candidate scan, and the chain the entry follows on the host.  Test infrastructure only - nothing here is
imported by the package.

A segment starts at a byte of a raw deflate stream.  It is a run of non-final blocks, stored (LEN / NLEN checked) or fixed
Huffman, up to and including the first empty stored block, behind which it ends on a byte.  A match reaches back to the
segment's own first output byte at the most; a segment makes at most SEGMENT_MAX output bytes and takes at most INPUT_MAX
input bytes.  The checks are made in the order of ``inf_segment``, so that refusals agree reason for reason and byte count
for byte count."""
import zlib

SEGMENT_MAX = 16384
# every byte a 9-bit literal (3 + 9 * 16384 + 7 + 3 bits, rounded up, + 4 = 18438), 8 further blocks of 5 bytes, rounded up to 16
INPUT_MAX = ((3 + 9 * SEGMENT_MAX + 7 + 3 + 7) // 8 + 4 + 8 * 5 + 15) // 16 * 16
OK, DYNAMIC, BTYPE3, FINAL, SYMBOL, NLEN, DISTANCE, OUTPUT, INPUT, END, CHAIN, SIZE = range(12)
REASONS = ('OK', 'DYNAMIC', 'BTYPE3', 'FINAL', 'SYMBOL', 'NLEN', 'DISTANCE', 'OUTPUT', 'INPUT', 'END', 'CHAIN', 'SIZE')
MARKER = b'\x00\x00\xff\xff'

_LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
_LEN_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
_DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
              8193, 12289, 16385, 24577)
_DIST_EXTRA = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)


def _rev(v: int, n: int) -> int:
    return int(format(v, f'0{n}b')[::-1], 2)


def _fixed_table():
    """9 stream bits (first bit lowest) -> (symbol, bits), from RFC 1951 3.2.6's table of code lengths."""
    table = [None] * 512
    for sym in range(288):
        if sym < 144:
            code, n = 0x30 + sym, 8
        elif sym < 256:
            code, n = 0x190 + sym - 144, 9
        elif sym < 280:
            code, n = sym - 256, 7
        else:
            code, n = 0xC0 + sym - 280, 8
        low = _rev(code, n)
        for hi in range(1 << (9 - n)):
            table[low | hi << n] = (sym, n)
    assert all(t is not None for t in table)
    return table


_FIXED = _fixed_table()


def decode_segment(data: bytes, start: int):
    """The segment of ``data`` that starts at byte ``start`` -> ``(end, out, reason)``: the byte behind it (-1 when it is
    refused), the bytes made (until the refusal) and OK or why it stopped.  Bits past the end of ``data`` read as 0."""
    data = bytes(data)
    p = 8 * start                                                 # the next bit
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

    while True:
        hdr = take(3)
        if p > limit:
            return stop(over())
        if hdr & 1:
            return stop(FINAL)
        if hdr >> 1 == 2:
            return stop(DYNAMIC)
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
        while True:
            sym, n = _FIXED[take(9)]
            p -= 9 - n
            if p > limit:
                return stop(over())
            if sym < 256:
                if len(out) >= SEGMENT_MAX:
                    return stop(OUTPUT)
                out.append(sym)
                continue
            if sym == 256:
                break
            if sym > 285:
                return stop(SYMBOL)
            length = _LEN_BASE[sym - 257] + take(_LEN_EXTRA[sym - 257])
            code = _rev(take(5), 5)
            if code > 29:
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


def marker_ends(data: bytes, lo: int = 0, hi: int = None):
    """The end of every 00 00 FF FF in ``data[lo:hi]`` (overlapping ones included), as positions in ``data``."""
    hi = len(data) if hi is None else hi
    found, at = [], data.find(MARKER, lo, hi)
    while at >= 0:
        found.append(at + 4)
        at = data.find(MARKER, at + 1, hi)
    return found


def candidates(stream: bytes):
    """What a caller hands to the entry for a stream: 0 and the end of every marker that lies below the stream's end."""
    return [0] + [e for e in marker_ends(stream) if e < len(stream)] if stream else []


def chain(stream: bytes, starts, out_bytes: int):
    """What ``fnn_inflate_segments`` reports -> ``(status, bytes or None, crc32)``."""
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


def full_flush_stream(data: bytes, level: int, k: int, strategy: int = zlib.Z_FIXED, flush: int = zlib.Z_FULL_FLUSH) -> bytes:
    """zlib's raw deflate of ``data``, flushed every ``k`` bytes (and behind the last ones) and not finished: with Z_FIXED and
    Z_FULL_FLUSH a chain of segments."""
    z = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
    return b''.join(z.compress(data[i:i + k]) + z.flush(flush) for i in range(0, len(data), k))


def inflate_raw(stream: bytes) -> bytes:
    """zlib's answer for a stream that is not finished: closed with the final empty fixed block."""
    d = zlib.decompressobj(-15)
    out = d.decompress(bytes(stream) + b'\x03\x00') + d.flush()
    assert d.eof and not d.unused_data
    return out


# ---------------------------------------------------------------------- data the tests share
def label_runs(n: int, elem: int = 1, seed: int = 0) -> bytes:
    """``n`` bytes of a label map of ``elem``-byte elements: runs of 1 .. 300 equal labels (2-byte maps: some above 255)."""
    import numpy as np
    rng = np.random.default_rng(seed)
    count = n // elem + 1
    reps = rng.integers(1, 300, count // 20 + 2)
    vals = rng.integers(0, 700 if elem == 2 else 200, reps.size)
    return np.repeat(vals, reps)[:count].astype('<u2' if elem == 2 else 'u1').tobytes()[:n]


def random_bytes(n: int, seed: int = 0) -> bytes:
    import numpy as np
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def texty_bytes(n: int, seed: int = 0) -> bytes:
    """Words drawn from a small vocabulary: zlib finds matches of many lengths and distances, overlapping ones among them."""
    import numpy as np
    rng = np.random.default_rng(seed)
    words = [bytes(rng.integers(97, 123, int(k), dtype=np.uint8)) for k in rng.integers(2, 9, 40)] + [b'aaaaaaaaaaaaaaaaaaaaaaaa', b'abababababababab']
    out = bytearray()
    while len(out) < n:
        out += words[int(rng.integers(0, len(words)))] + b' '
    return bytes(out[:n])
