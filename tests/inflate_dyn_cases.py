"""Inputs the tests of the dynamic-Huffman device inflate share (tests/test_inflate_dyn_cpu.py,
tests/test_inflate_dyn_core_host_cpu.py, tests/test_gpu_inflate_dyn.py): zlib's full-flush streams with the default strategy,
the project's own dynamic fragments, hand-made table headers - one per rule of csrc/inflate_dyn_core.h - and a corpus of
truncated and bit-flipped segments.  Test infrastructure only."""
import functools
import zlib

import numpy as np

import deflate_dyn_ref as dyn
import deflate_ref
import inflate_dyn_ref as ref

SEG = ref.SEGMENT_MAX
EMPTY_STORED = b'\x00\x00\xff\xff'


# ---------------------------------------------------------------------- streams that chain
def zlib_data():
    return {'texty': ref.texty_bytes(40000, 1), 'random': ref.random_bytes(20000, 2), 'runs1': ref.label_runs(40000, 1, 4),
            'runs2': ref.label_runs(40000, 2, 5)}


@functools.lru_cache(maxsize=None)
def zlib_streams():
    """name -> (stream, data): zlib's default strategy, Z_FULL_FLUSH every k bytes; levels 1, 6, 9, k = 100, 4096, 16384."""
    S = {}
    for name, data in zlib_data().items():
        for level in (1, 6, 9):
            for k in (100, 4096, SEG):
                d = data[:3000] if k == 100 else data
                S[f'zlib-{name}-l{level}-k{k}'] = (ref.full_flush_stream(d, level, k, zlib.Z_DEFAULT_STRATEGY), d)
    return S


FRAGMENT_SIZES = (1, 255, SEG, SEG + 1, 2 * SEG + 5, 5 * SEG + 77)


@functools.lru_cache(maxsize=None)
def project_fragments():
    """name -> (fragment, data, dynamic chunks): ``deflate_dyn_ref.fragment`` of label maps, and of the two chunks that reach
    the length limits of its codes."""
    S = {}
    for elem in (1, 2):
        for n in FRAGMENT_SIZES:
            data = ref.label_runs(n, elem, seed=n)
            S[f'labels{elem}-{n}'] = dyn.fragment(data, elem) + (data,)
    S['fibonacci'] = dyn.fragment(dyn.fibonacci_chunk(), 1) + (dyn.fibonacci_chunk(),)
    S['deep-header'] = dyn.fragment(dyn.deep_header_chunk(), 1) + (dyn.deep_header_chunk(),)
    return {k: (frag, data, n_dyn) for k, (frag, n_dyn, data) in S.items()}


@functools.lru_cache(maxsize=None)
def fixed_only_streams():
    """name -> (stream, data): streams without a dynamic block."""
    S = {}
    for elem in (1, 2):
        for n in (1, 255, SEG + 1):
            data = ref.label_runs(n, elem, seed=n)
            S[f'fixed-labels{elem}-{n}'] = (deflate_ref.fragment(data, elem), data)
    for name, data in (('texty', ref.texty_bytes(9000, 1)), ('random', ref.random_bytes(5000, 2))):
        for k in (100, 4096):
            d = data[:3000] if k == 100 else data
            S[f'fixed-zlib-{name}-k{k}'] = (ref.full_flush_stream(d, 9, k), d)
    return S


# ---------------------------------------------------------------------- hand-made table headers
# a complete code-length code over all 19 symbols: 13 of 4 bits and 6 of 5 (13 / 16 + 6 / 32 = 1)
CL_ALL = [4] * 13 + [5] * 6


def dyn_block(lit: dict, dist: dict, body, hlit=None, hdist=None, cl=None, coded=None, fields=None, tail=EMPTY_STORED + bytes(8)):
    """One non-final BTYPE 10 block, then the bits of an empty stored block.  ``lit`` / ``dist``: symbol -> code length.
    ``coded``: the length sequence as (code-length symbol, extra bits, their value), by default one length after the other.
    ``cl``: the 19 lengths of the code-length code.  ``fields``: the raw 5-, 5- and 4-bit fields in place of the counts.
    ``body``: ('L', symbol) / ('D', symbol) by the block's codes, ('B', value, bits) as they are."""
    hlit = max(257, max(lit) + 1) if hlit is None else hlit
    hdist = max(1, max(dist, default=0) + 1) if hdist is None else hdist
    lens = [lit.get(s, 0) for s in range(hlit)] + [dist.get(s, 0) for s in range(hdist)]
    cl = CL_ALL if cl is None else cl
    coded = [(v, 0, 0) for v in lens] if coded is None else coded
    b = deflate_ref._Bits()
    b.put(0, 1)
    b.put(2, 2)
    f = (hlit - 257, hdist - 1, 15) if fields is None else fields
    b.put(f[0], 5)
    b.put(f[1], 5)
    b.put(f[2], 4)
    for i in range(f[2] + 4):
        b.put(cl[dyn.ORDER[i]], 3)
    cl_codes = dyn.canonical(cl)
    for s, e, v in coded:
        b.huff(cl_codes[s], cl[s])
        b.put(v, e)
    codes = {'L': (dyn.canonical(lens[:hlit]), lens[:hlit]), 'D': (dyn.canonical(lens[hlit:]), lens[hlit:])}
    for item in body:
        if item[0] == 'B':
            b.put(item[1], item[2])
        else:
            c, n = codes[item[0]]
            assert n[item[1]], item
            b.huff(c[item[1]], n[item[1]])
    b.put(0, 3)
    b.to_byte()
    return bytes(b.out) + tail


def _plain(lens):
    return [(v, 0, 0) for v in lens]


@functools.lru_cache(maxsize=None)
def hand_made():
    """name -> (stream, reason, the bytes made by an accepted one).  Every stream is followed by 8 zero bytes or is a whole
    segment, so that no refusal is the input's end."""
    A, EOB = 97, 256
    two = {A: 1, EOB: 1}
    H = {}
    for field in (30, 31):
        H[f'hlit-{257 + field}'] = (dyn_block(two, {}, [], fields=(field, 0, 15)), ref.TABLES, None)
        H[f'hdist-{1 + field}'] = (dyn_block(two, {}, [], fields=(0, field, 15)), ref.TABLES, None)
    H['cl-incomplete'] = (dyn_block(two, {}, [], cl=[2, 2] + [0] * 17), ref.TABLES, None)
    H['cl-single'] = (dyn_block(two, {}, [], cl=[1] + [0] * 18), ref.TABLES, None)
    H['cl-empty'] = (dyn_block(two, {}, [], cl=[0] * 19), ref.TABLES, None)
    H['cl-oversubscribed'] = (dyn_block(two, {}, [], cl=[1, 1, 1] + [0] * 16), ref.TABLES, None)
    H['16-at-0'] = (dyn_block(two, {}, [], coded=[(16, 2, 0)] + _plain([0] * 255)), ref.TABLES, None)
    lens = [two.get(s, 0) for s in range(257)]
    H['run-overshoots'] = (dyn_block(two, {}, [], coded=_plain(lens) + [(17, 3, 0)]), ref.TABLES, None)
    H['run-overshoots-18'] = (dyn_block(two, {}, [], coded=_plain(lens[:200]) + [(18, 7, 127)]), ref.TABLES, None)
    H['no-end-of-block'] = (dyn_block({A: 1, 98: 1}, {}, [], hlit=257), ref.TABLES, None)
    H['lit-oversubscribed'] = (dyn_block({A: 1, 98: 1, EOB: 1}, {}, []), ref.TABLES, None)
    H['lit-incomplete'] = (dyn_block({A: 2, EOB: 2}, {}, []), ref.TABLES, None)
    H['dist-oversubscribed'] = (dyn_block(two, {0: 1, 1: 1, 2: 1}, []), ref.TABLES, None)
    H['dist-incomplete'] = (dyn_block(two, {0: 2, 1: 2}, []), ref.TABLES, None)
    H['only-end-of-block'] = (dyn_block({EOB: 1}, {}, [('L', EOB)], tail=EMPTY_STORED), ref.OK, b'')
    H['only-end-of-block-pattern-1'] = (dyn_block({EOB: 1}, {}, [('B', 1, 1)]), ref.SYMBOL, None)
    H['no-distances-literals'] = (dyn_block(two, {}, [('L', A), ('L', A), ('L', EOB)], tail=EMPTY_STORED), ref.OK, b'aa')
    with_length = {A: 2, EOB: 2, 257: 1}
    H['no-distances-length'] = (dyn_block(with_length, {}, [('L', A), ('L', 257), ('B', 0, 1), ('L', EOB)]), ref.SYMBOL, None)
    H['one-distance'] = (dyn_block(with_length, {0: 1}, [('L', A), ('L', 257), ('D', 0), ('L', EOB)], tail=EMPTY_STORED), ref.OK, b'aaaa')
    H['one-distance-pattern-1'] = (dyn_block(with_length, {0: 1}, [('L', A), ('L', 257), ('B', 1, 1), ('L', EOB)]), ref.SYMBOL, None)
    # 256 -> 1, then six zeros in one run: 257 .. 259 of the literal / length lengths and 0 .. 2 of the distance lengths
    crossing = _plain([two.get(s, 0) for s in range(257)]) + [(17, 3, 3), (1, 0, 0)]
    H['run-crosses'] = (dyn_block(two, {3: 1}, [('L', A), ('L', EOB)], hlit=260, hdist=4, coded=crossing, tail=EMPTY_STORED), ref.OK, b'a')
    # a repeat crosses too: 258 is 3 bits long and 16 repeats that for 259 and the distances 0 and 1
    rep, rep_dist = {A: 1, EOB: 2, 258: 3, 259: 3}, {0: 3, 1: 3, 2: 2, 3: 1}
    repeated = _plain([rep.get(s, 0) for s in range(259)]) + [(16, 2, 0), (2, 0, 0), (1, 0, 0)]
    H['repeat-crosses'] = (dyn_block(rep, rep_dist, [('L', A), ('L', 258), ('D', 0), ('L', EOB)], coded=repeated, tail=EMPTY_STORED), ref.OK, b'aaaaa')
    return H


# ---------------------------------------------------------------------- truncated and bit-flipped segments
@functools.lru_cache(maxsize=None)
def mutation_bases():
    """Whole segments of at most a few hundred bytes, most of them with a dynamic block."""
    bases = []
    for name in ('zlib-texty-l9-k100', 'zlib-runs2-l6-k100', 'zlib-random-l1-k100', 'zlib-runs1-l1-k100'):
        stream = zlib_streams()[name][0]
        at = 0
        while at < len(stream) and len(bases) < 40:
            end = ref.decode_segment(stream, at)[0]
            assert end > at
            if end - at <= 400:
                bases.append(stream[at:end])
            at = end
    for elem in (1, 2):
        frag, n_dyn = dyn.fragment(ref.label_runs(6000, elem, seed=9), elem)
        assert n_dyn == 1 and len(frag) <= 600
        bases.append(frag)
    bases += [s for s, reason, _ in hand_made().values() if reason == ref.OK]
    return bases


def mutated(n: int, seed: int = 20250117):
    """``n`` cases: a base segment cut short (one in four) or with one to three bits flipped, two flips in three within the
    first 80 bytes, where the table header lies."""
    rng = np.random.default_rng(seed)
    bases = mutation_bases()
    out = []
    for case in range(n):
        s = bytearray(bases[int(rng.integers(0, len(bases)))])
        if case % 4 == 0:
            s = s[:int(rng.integers(1, len(s) + 1))]
        else:
            for _ in range(int(rng.integers(1, 4))):
                hi = min(80, len(s)) if rng.integers(0, 3) else len(s)
                s[int(rng.integers(0, hi))] ^= 1 << int(rng.integers(0, 8))
        out.append(bytes(s))
    return out


def zlib_says(segment: bytes):
    """zlib's inflate on the segment closed with the final empty fixed block -> its bytes, or None where it raises or does
    not reach the end."""
    d = zlib.decompressobj(-15)
    try:
        out = d.decompress(segment + b'\x03\x00') + d.flush()
    except zlib.error:
        return None
    return out if d.eof else None
