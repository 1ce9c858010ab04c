"""A pure-Python restatement of the device deflate encoder with per-chunk dynamic Huffman tables (csrc/deflate_dyn.hip,
csrc/deflate_dyn_core.h), on top of the tokens of tests/deflate_ref.py.  Test infrastructure only.

A chunk (CHUNK input bytes, tokenised segment by segment as in deflate_ref) is one non-final block, its end-of-block code and
an empty stored block.  The block is BTYPE 10 with the chunk's own tables where that takes fewer bits than BTYPE 01, the fixed
code of deflate_ref; a tie goes to the fixed code.

* Frequencies: the literal / length symbols of the chunk's tokens, and one for 256.  A non-empty chunk uses at least two
  symbols (the first byte of a segment is a literal; 256).
* The distance code is constant: symbols 0 and 1 of length 1 (HDIST = 2), so a match's distance costs one bit.
* ``code_lengths(freq, limit)``: a Huffman tree from two queues - the used symbols ascending by (frequency, index), and the
  merged nodes in the order they are made; the smaller head is taken, the merged node on a tie.  Leaf depths above ``limit``
  count as ``limit``; while the Kraft sum exceeds 1, the deepest leaf above the last level moves one level down and a leaf of
  the last level becomes its brother (2^-limit less).  The lengths go longest first to the symbols in ascending order.
  (Complete, not claimed to be the optimal length-limited code.)
* Codes are canonical (RFC 1951 3.2.2).  HLIT = max(257, last used symbol + 1).
* The HLIT + 2 lengths (literal / length, then the two distance lengths, as one sequence: a run may cross from the one into
  the other) are coded greedily from the left.  At position i with value v and r equal values from i on:
  v = 0: r >= 11 -> 18 with min(r, 138); r >= 3 -> 17 with r; else the length 0 itself.
  v > 0: i > 0, the value before i is v and r >= 3 -> 16 with min(r, 6); else the length v itself.
* The code-length code is ``code_lengths(., 7)``; HCLEN is trimmed along the permuted order and is at least 4.
"""
import functools
from collections import deque

import deflate_ref as R

ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
NLIT, NCL = 286, 19
LIT_LIMIT, CL_LIMIT = 15, 7


def length_symbol(length: int):
    """-> (symbol, extra bits, their value) of a match length."""
    k = max(i for i in range(29) if R._LEN_BASE[i] <= length)
    return 257 + k, R._LEN_EXTRA[k], length - R._LEN_BASE[k]


def huffman_depths(freq):
    """The leaf depths of the two-queue Huffman tree over the ``freq`` (all non-zero, ascending; two or more)."""
    leaves, merged, depths = deque((f, i) for i, f in enumerate(freq)), deque(), [0] * len(freq)

    def take():
        if leaves and (not merged or leaves[0][0] < merged[0][0]):
            return leaves.popleft()
        return merged.popleft()

    while len(leaves) + len(merged) > 1:
        a, b = take(), take()
        merged.append((a[0] + b[0], (a[1], b[1])))                # a tree is a leaf's index or a pair of trees
    stack = [(merged[0][1], 0)]
    while stack:
        tree, depth = stack.pop()
        if isinstance(tree, tuple):
            stack += [(tree[0], depth + 1), (tree[1], depth + 1)]
        else:
            depths[tree] = depth
    return depths


def code_lengths(freq, limit: int):
    lens = [0] * len(freq)
    used = sorted((f, s) for s, f in enumerate(freq) if f)
    if len(used) == 1:
        lens[used[0][1]] = 1
    if len(used) < 2:
        return lens
    have = [min(d, limit) for d in huffman_depths([f for f, _ in used])]
    while sum(2 ** (limit - d) for d in have) > 2 ** limit:
        moved = max(d for d in have if d < limit)                 # this leaf moves one level down ...
        have.remove(moved)
        have.remove(limit)                                        # ... and a leaf of the last level becomes its brother
        have += [moved + 1, moved + 1]
    for (_, s), d in zip(used, sorted(have, reverse=True)):
        lens[s] = d
    return lens


def canonical(lens):
    """RFC 1951 3.2.2: -> the code of every symbol (most significant bit first)."""
    count = [0] * (max(lens) + 2)
    for n in lens:
        count[n] += n > 0
    nxt, code = [0] * len(count), 0
    for bits in range(1, len(count)):
        code = (code + count[bits - 1]) << 1
        nxt[bits] = code
    codes = [0] * len(lens)
    for s, n in enumerate(lens):
        if n:
            codes[s] = nxt[n]
            nxt[n] += 1
    return codes


def run_length(seq):
    """The greedy 16 / 17 / 18 coding: -> [(symbol, extra bits, their value)]."""
    out, i = [], 0
    while i < len(seq):
        v, r = seq[i], 1
        while i + r < len(seq) and seq[i + r] == v:
            r += 1
        if v == 0 and r >= 11:
            r = min(r, 138)
            out.append((18, 7, r - 11))
        elif v == 0 and r >= 3:
            out.append((17, 3, r - 3))
        elif v and i and seq[i - 1] == v and r >= 3:
            r = min(r, 6)
            out.append((16, 2, r - 3))
        else:
            r = 1
            out.append((v, 0, 0))
        i += r
    return out


def chunk_symbols(chunk: bytes, elem_bytes: int):
    """The chunk's tokens as (symbol, extra bits, their value, whether a distance follows), the end-of-block symbol last."""
    out = []
    for s in range(0, len(chunk), R.SEGMENT):
        for kind, v in R.tokens(chunk[s:s + R.SEGMENT], elem_bytes):
            out.append((v, 0, 0, False) if kind == 'lit' else length_symbol(v) + (True,))
    out.append((256, 0, 0, False))
    return out


def fixed_length(sym: int) -> int:
    return 8 if sym < 144 else 9 if sym < 256 else 7 if sym < 280 else 8


def tables(syms):
    """-> (the literal / length lengths, HLIT, the run-length coded header, the code-length code's lengths, HCLEN, the bits
    of the table header behind BTYPE)."""
    freq = [0] * NLIT
    for s, _, _, _ in syms:
        freq[s] += 1
    lens = code_lengths(freq, LIT_LIMIT)
    hlit = max(257, max(s for s in range(NLIT) if lens[s]) + 1)
    coded = run_length(lens[:hlit] + [1, 1])
    clfreq = [0] * NCL
    for s, _, _ in coded:
        clfreq[s] += 1
    cllens = code_lengths(clfreq, CL_LIMIT)
    hclen = max(4, max(i for i in range(NCL) if cllens[ORDER[i]]) + 1)
    bits = 5 + 5 + 4 + 3 * hclen + sum(cllens[s] + e for s, e, _ in coded)
    return lens, hlit, coded, cllens, hclen, bits


def chunk_bytes(chunk: bytes, elem_bytes: int):
    """-> (the chunk's bytes, whether it took its own tables)."""
    syms = chunk_symbols(chunk, elem_bytes)
    lens, hlit, coded, cllens, hclen, head = tables(syms)
    fixed = sum(fixed_length(s) + e + (5 if m else 0) for s, e, _, m in syms)
    dynamic = head + sum(lens[s] + e + (1 if m else 0) for s, e, _, m in syms)
    if dynamic >= fixed:
        return R.chunk_bytes(chunk, elem_bytes), False
    b = R._Bits()
    b.put(0, 1)                                                   # BFINAL = 0
    b.put(2, 2)                                                   # BTYPE = 10
    b.put(hlit - 257, 5)
    b.put(1, 5)                                                   # HDIST = 2
    b.put(hclen - 4, 4)
    for i in range(hclen):
        b.put(cllens[ORDER[i]], 3)
    clcodes = canonical(cllens)
    for s, e, v in coded:
        b.huff(clcodes[s], cllens[s])
        b.put(v, e)
    codes = canonical(lens)
    for s, e, v, m in syms:
        b.huff(codes[s], lens[s])
        b.put(v, e)
        if m:
            b.put(elem_bytes - 1, 1)                              # distance code 0 or 1, one bit
    b.put(0, 3)                                                   # BFINAL = 0, BTYPE = 00 ...
    b.to_byte()
    b.out += b'\x00\x00\xff\xff'                                  # ... of length 0
    return bytes(b.out), True


@functools.lru_cache(maxsize=None)
def _fragment(data: bytes, elem_bytes: int):
    made = [chunk_bytes(data[c:c + R.CHUNK], elem_bytes) for c in range(0, len(data), R.CHUNK)]
    return b''.join(m[0] for m in made), sum(m[1] for m in made)


def fragment(data: bytes, elem_bytes: int):
    """-> (the device's fragment for the file's voxel bytes ``data`` of ``elem_bytes``-byte elements, the number of chunks
    that took their own tables).  Computed once per input."""
    return _fragment(bytes(data), elem_bytes)


# ---------------------------------------------------------------------- inputs the tests share
def fibonacci_chunk() -> bytes:
    """19 literals whose frequencies are the Fibonacci numbers 1, 1, 2, ... 4181 - 10 945 bytes, no two equal neighbours, so
    every token is a literal: a Huffman code of these frequencies (and the 1 of symbol 256) is 19 deep."""
    fib = [1, 1]
    while len(fib) < 19:
        fib.append(fib[-1] + fib[-2])
    return _without_equal_neighbours({10 + i: f for i, f in enumerate(fib)})


def _without_equal_neighbours(counts: dict) -> bytes:
    """``counts[v]`` times the byte v, no two equal neighbours (no count exceeds half of all)."""
    n = sum(counts.values())
    values = [v for v, c in sorted(counts.items(), key=lambda t: -t[1]) for _ in range(c)]   # the most frequent first ...
    out = bytearray(n)
    for v, p in zip(values, list(range(0, n, 2)) + list(range(1, n, 2))):      # ... onto the even places, then the odd ones
        out[p] = v
    assert all(a != b for a, b in zip(out, out[1:]))
    return bytes(out)


def deep_header_chunk() -> bytes:
    """A chunk found by a random search (seed 173 of 200): 167 literals with skewed frequencies, 16 080 bytes, no two equal
    neighbours.  Its table header uses 13 code-length symbols so unevenly that their Huffman tree is 9 deep: the 7-bit
    limit of the code-length code applies."""
    import numpy as np
    rng = np.random.default_rng(173)
    k = int(rng.integers(3, 200))
    w = rng.random(k) ** int(rng.integers(1, 12))
    return _without_equal_neighbours({int(s): 1 + int(x * 16000) for s, x in zip(rng.choice(256, k, replace=False), w / w.sum())})


def header_code_frequencies(chunk: bytes, elem_bytes: int):
    """The frequencies of the 19 code-length symbols in the chunk's table header."""
    clfreq = [0] * NCL
    for s, _, _ in tables(chunk_symbols(chunk, elem_bytes))[2]:
        clfreq[s] += 1
    return clfreq


TINY_CHUNK = b'\x01\x02\x03\x02\x01'                            # a table header costs more than these bytes save
