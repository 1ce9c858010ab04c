"""A pure-Python restatement of the device deflate encoder (csrc/deflate.hip): its token rule, its bit packing and the
CRC-32 combine.  Test infrastructure only - nothing here is imported by the package.

The fragment for ``data`` (the voxel bytes as the file holds them) is a concatenation of independent chunks of CHUNK
input bytes.  A chunk is one non-final fixed-Huffman block (RFC 1951 3.2.6) followed by an empty stored block, so that it
ends on a byte.  Inside a chunk every SEGMENT bytes are tokenised on their own, in order:

* at position p of a segment, m = the number of bytes from p on that equal the byte one element (``elem_bytes``) before
  them, not counted past the segment's end nor past 258, and 0 when p < elem_bytes (the source lies inside the segment);
* m >= 3: a match of length m and distance elem_bytes, and p += m; otherwise the literal ``seg[p]`` and p += 1.
"""
import zlib

SEGMENT = 256
CHUNK = 16384
POLY = 0xEDB88320                                                 # CRC-32, reflected

_LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
_LEN_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)


def bound(n_bytes: int) -> int:
    """What ``fnn_deflate_bound`` returns: every byte a 9-bit literal, and per chunk 13 bits of block framing rounded up
    to a byte plus the four bytes of the stored block."""
    if n_bytes <= 0:
        return 0
    return (9 * n_bytes + 7) // 8 + 6 * ((n_bytes + CHUNK - 1) // CHUNK)


class _Bits:
    """Deflate's bit order: values from the least significant bit of each byte up, Huffman codes most significant bit first."""

    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, value: int, nbits: int):
        self.acc |= value << self.n
        self.n += nbits
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def huff(self, code: int, nbits: int):
        self.put(int(format(code, f'0{nbits}b')[::-1], 2), nbits)

    def symbol(self, sym: int):
        """A literal / length symbol of the fixed code."""
        if sym < 144:
            self.huff(0x30 + sym, 8)
        elif sym < 256:
            self.huff(0x190 + sym - 144, 9)
        elif sym < 280:
            self.huff(sym - 256, 7)
        else:
            self.huff(0xC0 + sym - 280, 8)

    def match(self, length: int, distance: int):
        k = max(i for i in range(29) if _LEN_BASE[i] <= length)
        self.symbol(257 + k)
        self.put(length - _LEN_BASE[k], _LEN_EXTRA[k])
        assert distance in (1, 2)                                 # distance codes 0 and 1: five bits, no extra bits
        self.huff(distance - 1, 5)

    def to_byte(self):
        if self.n:
            self.put(0, 8 - self.n)


def tokens(seg: bytes, elem_bytes: int):
    """The tokens of one segment: ``('lit', value)`` or ``('match', length)``."""
    p, n, out = 0, len(seg), []
    while p < n:
        m = 0
        if p >= elem_bytes:
            while p + m < n and m < 258 and seg[p + m] == seg[p + m - elem_bytes]:
                m += 1
        if m >= 3:
            out.append(('match', m))
            p += m
        else:
            out.append(('lit', seg[p]))
            p += 1
    return out


def chunk_bytes(chunk: bytes, elem_bytes: int) -> bytes:
    b = _Bits()
    b.put(0, 1)                                                   # BFINAL = 0
    b.put(1, 2)                                                   # BTYPE = 01
    for s in range(0, len(chunk), SEGMENT):
        for kind, v in tokens(chunk[s:s + SEGMENT], elem_bytes):
            if kind == 'lit':
                b.symbol(v)
            else:
                b.match(v, elem_bytes)
    b.symbol(256)                                                 # end of block
    b.put(0, 3)                                                   # BFINAL = 0, BTYPE = 00 ...
    b.to_byte()
    b.out += b'\x00\x00\xff\xff'                                  # ... of length 0
    return bytes(b.out)


def fragment(data: bytes, elem_bytes: int) -> bytes:
    """The device's fragment for the file's voxel bytes ``data`` of ``elem_bytes``-byte elements."""
    data = bytes(data)
    return b''.join(chunk_bytes(data[c:c + CHUNK], elem_bytes) for c in range(0, len(data), CHUNK))


def inflate(frag: bytes) -> bytes:
    """The bytes a raw-deflate decoder reads from the fragment closed by the final empty fixed block."""
    d = zlib.decompressobj(-15)
    out = d.decompress(frag + b'\x03\x00') + d.flush()
    assert d.eof and not d.unused_data
    return out


# ---------------------------------------------------------------------- CRC-32 combine
def mulmod(a: int, b: int) -> int:
    """a * b modulo the CRC-32 polynomial, both in the reflected representation (bit 31 is x^0)."""
    p = 0
    for i in range(32):
        if a & (0x80000000 >> i):
            p ^= b
        b = (b >> 1) ^ (POLY if b & 1 else 0)
    return p


def xpow8(n_bytes: int) -> int:
    """x^(8 n_bytes) by repeated squaring."""
    r, sq, e = 0x80000000, 0x40000000, 8 * n_bytes               # x^0, x^1
    while e:
        if e & 1:
            r = mulmod(r, sq)
        sq = mulmod(sq, sq)
        e >>= 1
    return r


def crc_combine(crc_a: int, crc_b: int, len_b: int) -> int:
    """zlib.crc32(A + B) from zlib.crc32(A), zlib.crc32(B) and len(B)."""
    return mulmod(crc_a, xpow8(len_b)) ^ crc_b
