"""Inputs the tests of the speculative device inflate share (tests/test_inflate_any_cpu.py,
tests/test_inflate_any_core_host_cpu.py, tests/test_gpu_inflate_any.py): raw deflate streams made with Python's zlib at test
time - no zlib version is assumed - the project's own fragments closed with 03 00, hand-made streams and a corpus of
truncated and bit-flipped ones.  Test infrastructure only.

The matrix is not the full cross of data, settings and sizes (about a thousand streams, which no suite could afford): every
kind of data meets every compression setting at one size that spans more than two windows (65541; 98304 for the tripled
random block), and every size meets the settings that change the block structure most - level 6 with memLevel 1 (a block
every 128 symbols), memLevel 8 (zlib's default) and level 0 (stored only) - on the two kinds of data at the extremes, label
runs and random bytes.  The 300000-byte streams are the label runs and the CT-like walk at memLevel 1 and 8."""
import functools
import zlib

import numpy as np

import deflate_dyn_ref as dyn
import deflate_ref
import inflate_any_ref as ref
import inflate_dyn_cases as dyn_cases
from inflate_ref import label_runs, random_bytes, texty_bytes

SIZES = (0, 1, 255, 32767, 32768, 32769, 65541, 300000)
FINAL_EMPTY = b'\x03\x00'


def ct_walk(n: int, seed: int = 3) -> bytes:
    """``n`` bytes of a CT-like int16 volume: a random walk with small steps around -1000 .. 1000."""
    rng = np.random.default_rng(seed)
    steps = rng.integers(-12, 13, n // 2 + 1)
    return np.clip(np.cumsum(steps) - 300, -1024, 3000).astype('<i2').tobytes()[:n]


def tripled_random() -> bytes:
    """3 x the same random 32768 bytes: matches at distance exactly 32768."""
    return random_bytes(32768, 11) * 3


def data_of(kind: str, n: int) -> bytes:
    return {'runs1': lambda: label_runs(n, 1, 4), 'runs2': lambda: label_runs(n, 2, 5), 'ct': lambda: ct_walk(n),
            'texty': lambda: texty_bytes(n, 1), 'random': lambda: random_bytes(n, 2), 'tripled': tripled_random}[kind]()


KINDS = ('runs1', 'runs2', 'ct', 'texty', 'random', 'tripled')
STRATEGIES = {'default': zlib.Z_DEFAULT_STRATEGY, 'filtered': zlib.Z_FILTERED, 'rle': zlib.Z_RLE, 'huffman': zlib.Z_HUFFMAN_ONLY,
              'fixed': zlib.Z_FIXED}
FLUSHES = {'sync': zlib.Z_SYNC_FLUSH, 'partial': getattr(zlib, 'Z_PARTIAL_FLUSH', 1), 'full': zlib.Z_FULL_FLUSH}


def deflate_raw(data: bytes, level: int, mem: int = 8, strategy: str = 'default', flush: str = None, every: int = 1000) -> bytes:
    z = zlib.compressobj(level, zlib.DEFLATED, -15, mem, STRATEGIES[strategy])
    if flush is None:
        return z.compress(data) + z.flush()
    return b''.join(z.compress(data[i:i + every]) + z.flush(FLUSHES[flush]) for i in range(0, len(data), every)) + z.flush()


def settings():
    """name -> keyword arguments of ``deflate_raw``."""
    S = {f'l{level}-m{mem}': dict(level=level, mem=mem) for level in (1, 6, 9) for mem in (1, 3, 8)}
    S.update({f'l6-{s}': dict(level=6, strategy=s) for s in ('filtered', 'rle', 'huffman', 'fixed')})
    S['l0'] = dict(level=0)
    S.update({f'l6-{f}flush': dict(level=6, flush=f) for f in FLUSHES})
    return S


@functools.lru_cache(maxsize=None)
def matrix():
    """name -> (stream, data)."""
    M = {}
    for kind in KINDS:
        data = data_of(kind, 65541)
        for name, kw in settings().items():
            M[f'{kind}-65541-{name}'] = (deflate_raw(data, **kw), data)
    for kind in ('runs1', 'random'):
        for n in SIZES[:-2]:
            data = data_of(kind, n)
            for name in ('l6-m1', 'l6-m8', 'l0'):
                M[f'{kind}-{n}-{name}'] = (deflate_raw(data, **settings()[name]), data)
    for kind in ('runs1', 'runs2', 'ct'):
        data = data_of(kind, 300000)
        for name in ('l6-m1', 'l6-m8'):
            M[f'{kind}-300000-{name}'] = (deflate_raw(data, **settings()[name]), data)
    for elem in (1, 2):
        for n in (1, 255, 32769, 65541):
            data = label_runs(n, elem, seed=n)
            M[f'own-fixed{elem}-{n}'] = (deflate_ref.fragment(data, elem) + FINAL_EMPTY, data)
            M[f'own-dynamic{elem}-{n}'] = (dyn.fragment(data, elem)[0] + FINAL_EMPTY, data)
    return M


def small(limit: int = 8192):
    """The matrix streams of at most ``limit`` compressed bytes."""
    return {k: v for k, v in matrix().items() if len(v[0]) <= limit}


# ---------------------------------------------------------------------- hand-made streams
def _fixed_block(tokens, final=False, btype=1) -> deflate_ref._Bits:
    b = deflate_ref._Bits()
    b.put(1 if final else 0, 1)
    b.put(btype, 2)
    for t in tokens:
        if isinstance(t, int):
            b.symbol(t)
        else:
            b.match(*t)
    b.symbol(256)
    return b


@functools.lru_cache(maxsize=None)
def hand_made():
    """name -> (stream, out_bytes, status, bytes or None)."""
    A, B, EOB = 97, 98, 256
    H = {}
    # a match that reaches before byte 0 of the stream: one literal, then 3 bytes from 2 back
    b = _fixed_block([A, (3, 2)], final=True)
    b.to_byte()
    H['before-byte-0'] = (bytes(b.out), 4, ref.DISTANCE, None)
    # four members, each a dynamic block and an empty stored block: 'ab'; a match that reaches 2 before its member (markers)
    # and one that copies those markers inside it; two members more that each reach back into the one before
    with_length = {A: 2, EOB: 2, 257: 1}
    reach = [('L', 257), ('D', 1), ('L', 257), ('D', 2), ('L', EOB)]                      # 3 from 2 back, 3 from 3 back
    blocks = [dyn_cases.dyn_block({A: 2, B: 2, EOB: 1}, {}, [('L', A), ('L', B), ('L', EOB)], tail=dyn_cases.EMPTY_STORED)]
    blocks += [dyn_cases.dyn_block(with_length, {1: 1, 2: 1}, reach, tail=dyn_cases.EMPTY_STORED) for _ in range(3)]
    stream = b''.join(blocks) + FINAL_EMPTY
    made = zlib.decompress(stream, -15)
    assert len(made) == 20
    H['marker-through-members'] = (stream, len(made), ref.OK, made)
    # BTYPE 3 behind a whole fixed block
    b = _fixed_block([A, B, A, B])
    b.put(0, 1)
    b.put(3, 2)
    b.to_byte()
    H['btype3-mid-stream'] = (bytes(b.out) + bytes(4), 4, ref.BTYPE3, None)
    # a final block that is not the input's end
    b = _fixed_block([A], final=True)
    b.to_byte()
    H['bytes-behind-final'] = (bytes(b.out) + b'\x00\x00', 1, ref.FINAL, None)
    return H


# ---------------------------------------------------------------------- truncated and bit-flipped streams
@functools.lru_cache(maxsize=None)
def mutation_bases():
    """Whole streams of at most 700 bytes with several members."""
    bases = [deflate_raw(label_runs(n, e, seed=n), 6, 1) for n in (3000, 9000) for e in (1, 2)]
    bases += [deflate_raw(ct_walk(400), 6, 1), deflate_raw(texty_bytes(900, 5), 9, 1), deflate_raw(texty_bytes(600, 6), 6, 8, 'fixed'),
              deflate_raw(random_bytes(300, 7), 0), hand_made()['marker-through-members'][0]]
    assert all(len(b) <= 700 for b in bases), [len(b) for b in bases]
    return bases


def mutated(n: int, seed: int = 20250321):
    """``n`` cases ``(stream, out_bytes)``: a base cut short (one in four) or with one to three bits flipped, as
    ``inflate_dyn_cases.mutated``; out_bytes is the base's."""
    rng = np.random.default_rng(seed)
    bases = mutation_bases()
    out = []
    for case in range(n):
        base = bases[int(rng.integers(0, len(bases)))]
        s = bytearray(base)
        if case % 4 == 0:
            s = s[:int(rng.integers(1, len(s) + 1))]
        else:
            for _ in range(int(rng.integers(1, 4))):
                hi = min(80, len(s)) if rng.integers(0, 3) else len(s)
                s[int(rng.integers(0, hi))] ^= 1 << int(rng.integers(0, 8))
        out.append((bytes(s), len(zlib.decompress(base, -15))))
    return out
