"""The device inflate without a GPU: the Python model of the segment rule and the chain (tests/inflate_ref.py) against zlib,
its refusals, ``imageio.chunked_layout`` on files of both kinds, the entry's declaration and what it refuses before it
touches the device (return code and exact ``fnn_last_error`` text, in the style of tests/test_entry_refusals_cpu.py)."""
import ctypes as C
import gzip
import os
import re
import struct
import zlib

import numpy as np
import pytest

import deflate_masks_ref as masks_ref
import deflate_ref
import inflate_ref as ref
from fast_nnunet_amd import capi, imageio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEG = ref.SEGMENT_MAX


# ---------------------------------------------------------------------- the model against zlib
@pytest.mark.parametrize('elem', (1, 2))
@pytest.mark.parametrize('n', (0, 1, 255, 256, 257, SEG - 1, SEG, SEG + 1, 3 * SEG + 5))
def test_model_inflates_the_label_encoders_fragments(n, elem):
    for data in (bytes(n), ref.label_runs(n, elem, seed=n), ref.random_bytes(n, seed=n)):
        frag = deflate_ref.fragment(data, elem)
        assert ref.chain(frag, ref.candidates(frag), len(data)) == (ref.OK, data, zlib.crc32(data))
        assert deflate_ref.inflate(frag) == data


def test_model_inflates_the_mask_encoders_fragments():
    m = (np.arange(3 * SEG + 77) // 37 % 5).astype(np.uint8)
    m[SEG + 700:SEG + 900] = 6
    for label in (2, 6, 9):                                        # everywhere; in one chunk (zero chunks around it); nowhere
        frag, mask = masks_ref.mask_fragment(m, label), masks_ref.mask_of(m, label).tobytes()
        assert ref.chain(frag, ref.candidates(frag), len(mask)) == (ref.OK, mask, zlib.crc32(mask))


@pytest.mark.parametrize('level', (1, 6, 9))
@pytest.mark.parametrize('k', (100, 4096, SEG))
def test_model_inflates_zlibs_fixed_full_flush_streams(level, k):
    """Checked here: Z_FIXED with Z_FULL_FLUSH every k <= 16384 bytes is a chain of segments - fixed-Huffman blocks with
    matches of general distance, on random bytes stored blocks with data - and every marker zlib wrote is a candidate."""
    for data in (ref.texty_bytes(3000 if k == 100 else 40000, 1), ref.random_bytes(3000 if k == 100 else 20000, 2), ref.label_runs(40000, 2, 5)):
        stream = ref.full_flush_stream(data, level, k)
        d = zlib.decompressobj(-15)
        assert d.decompress(stream) == data and not d.eof
        assert ref.chain(stream, ref.candidates(stream), len(data)) == (ref.OK, data, zlib.crc32(data))
        assert len(ref.candidates(stream)) >= (len(data) + k - 1) // k
    assert ref.full_flush_stream(ref.random_bytes(5000, 2), level, k)[0] & 7 == 0, 'random bytes: a stored block'


def test_model_takes_false_candidates_and_ignores_them():
    data = ref.texty_bytes(3000, 1)
    stream = ref.full_flush_stream(data, 9, 100)
    assert ref.chain(stream, list(range(len(stream))), len(data)) == (ref.OK, data, zlib.crc32(data))


def test_model_refuses_with_the_reason():
    texty = ref.texty_bytes(40000, 1)

    def said(stream, out_bytes=len(texty), starts=None):
        return ref.REASONS[ref.chain(stream, ref.candidates(stream) if starts is None else starts, out_bytes)[0]]

    assert said(ref.full_flush_stream(texty, 6, 4096, zlib.Z_DEFAULT_STRATEGY)) == 'DYNAMIC'
    assert said(ref.full_flush_stream(texty, 6, 4096, flush=zlib.Z_SYNC_FLUSH)) == 'DISTANCE'       # distances cross the segments
    assert said(ref.full_flush_stream(texty, 1, SEG + 1)) == 'OUTPUT'
    a = ref.full_flush_stream(texty[:1000], 1, 1000)
    z = zlib.compressobj(1, zlib.DEFLATED, -15, 8, zlib.Z_FIXED)
    assert said(a + z.compress(texty[1000:2000]) + z.flush() + a, 3000) == 'FINAL'
    good = ref.full_flush_stream(texty, 1, 4096)
    assert said(good[:-3]) == 'END'
    assert said(good + b'\x01\x02\x03', starts=ref.candidates(good)) == 'CHAIN'
    assert said(good, len(texty) + 1) == said(good, len(texty) - 1) == 'SIZE'
    assert said(good) == 'OK'
    # single segments: a bad NLEN, BTYPE 3, symbols outside the code, the input budget
    assert ref.decode_segment(b'\x00\x05\x00\xfa\xfe', 0)[2] == ref.NLEN
    assert ref.decode_segment(b'\x06\x00\x00\x00\x00', 0)[2] == ref.BTYPE3
    bits = deflate_ref._Bits()
    bits.put(2, 3)
    bits.huff(0xC0 + 6, 8)                                        # literal / length symbol 286
    bits.to_byte()
    assert ref.decode_segment(bytes(bits.out) + bytes(8), 0)[2] == ref.SYMBOL
    bits = deflate_ref._Bits()
    bits.put(2, 3)
    bits.symbol(65)
    bits.symbol(257)
    bits.huff(30, 5)                                              # distance symbol 30
    bits.to_byte()
    assert ref.decode_segment(bytes(bits.out) + bytes(8), 0)[2] == ref.SYMBOL
    bits = deflate_ref._Bits()
    for _ in range(8 * ref.INPUT_MAX // 10 + 2):                  # empty fixed blocks, 10 bits each, past the budget
        bits.put(2, 3)
        bits.symbol(256)
    bits.to_byte()
    assert ref.decode_segment(bytes(bits.out) + bytes(8), 0)[1:] == (b'', ref.INPUT)
    assert ref.INPUT_MAX == 18480


# ---------------------------------------------------------------------- chunked_layout
def _device_style_file(seg: np.ndarray) -> bytes:
    data = seg.astype('<u2' if seg.dtype.itemsize == 2 else 'u1').tobytes()
    labels = imageio.DeviceCompressedLabels(deflate_ref.fragment(data, seg.dtype.itemsize), zlib.crc32(data), len(data), seg.shape,
                                            seg.dtype.itemsize == 2, np.diag([1.5, 2.0, 2.5, 1.0]))
    return imageio.compressed_label_file_bytes(labels)


@pytest.mark.parametrize('name', ['example_ct_sm.nii.gz', 'example_ct_sm_T300_output.nii.gz'])
def test_chunked_layout_is_none_for_zlibs_files(golden_dir, name):
    path = os.path.join(golden_dir, name)
    assert imageio.chunked_layout(open(path, 'rb').read(), imageio.read_header(path)) is None


@pytest.mark.parametrize('dtype', ['u1', '<u2'])
def test_chunked_layout_of_a_device_written_file(dtype):
    seg = (np.arange(31 * 40 * 50) // 93 % 7 * (90 if dtype == '<u2' else 1)).astype(dtype).reshape(31, 40, 50)
    blob = _device_style_file(seg)
    plain = gzip.decompress(blob)
    hdr = imageio.NiftiHeader(plain[:352])
    lay = imageio.chunked_layout(blob, hdr)
    assert lay is not None
    head_z = blob[10:lay.first]
    assert head_z.endswith(b'\x00\x00\xff\xff') and ref.inflate_raw(head_z) == plain[:352]
    assert lay.header_crc == zlib.crc32(plain[:352]) and lay.crc32 == zlib.crc32(plain)
    stream = blob[lay.first:lay.first + lay.in_bytes]
    assert stream == deflate_ref.fragment(plain[352:], seg.dtype.itemsize) and blob[lay.first + lay.in_bytes:-8] == b'\x03\x00'
    assert lay.starts.dtype == np.int64 and lay.starts.tolist() == ref.candidates(stream)
    assert len(lay.starts) >= (seg.nbytes + SEG - 1) // SEG
    status, made, crc = ref.chain(stream, lay.starts.tolist(), hdr.n_bytes)
    assert (status, made) == (ref.OK, plain[352:])
    assert imageio.crc32_combine(lay.header_crc, crc, hdr.n_bytes) == lay.crc32


def test_chunked_layout_is_none_for_an_altered_file():
    seg = (np.arange(9 * 10 * 11) // 7 % 4).astype(np.uint8).reshape(9, 10, 11)
    blob = bytearray(_device_style_file(seg))
    hdr = imageio.NiftiHeader(gzip.decompress(bytes(blob))[:352])
    assert imageio.chunked_layout(bytes(blob), hdr) is not None

    def altered(at, value):
        b = bytearray(blob)
        b[at] = value
        return imageio.chunked_layout(bytes(b), hdr)

    assert altered(len(blob) - 4, blob[-4] ^ 1) is None            # ISIZE
    assert altered(3, 8) is None                                   # FLG: a file name would follow
    assert altered(2, 7) is None                                   # CM
    assert altered(len(blob) - 12, 0xFE) is None                   # the marker in front of 03 00
    assert altered(len(blob) - 10, 0x01) is None                   # the final block
    assert imageio.chunked_layout(bytes(blob[:20]), hdr) is None
    # a header segment that does not inflate to vox_offset bytes: none is found
    other = imageio.NiftiHeader(gzip.decompress(bytes(blob))[:352])
    other.vox_offset += 16
    other_isize = bytearray(blob)
    other_isize[-4:] = struct.pack('<I', other.vox_offset + other.n_bytes)
    assert imageio.chunked_layout(bytes(other_isize), other) is None


# ---------------------------------------------------------------------- the entry
def test_entry_is_declared_exported_and_additive():
    header = open(os.path.join(ROOT, 'include', 'fnn.h')).read()
    lib = capi.load_library()
    assert re.search(r'\bfnn_inflate_segments\s*\(', header) and 'fnn_inflate_segments' in capi.EXPORTS and hasattr(lib, 'fnn_inflate_segments')
    assert '#define FNN_ABI_VERSION 4' in header and lib.fnn_abi_version() == 4
    for value, name in enumerate(ref.REASONS):
        assert re.search(rf'#define FNN_INFLATE_{name} {value}\b', header) and getattr(capi, 'FNN_INFLATE_' + name) == value
    assert capi.INFLATE_REASONS == ref.REASONS
    assert re.search(r'#define FNN_INFLATE_SEGMENT_MAX 16384\b', header) and capi.FNN_INFLATE_SEGMENT_MAX == ref.SEGMENT_MAX


_HOST = np.zeros(1 << 14, np.uint8)
_BASE = (_HOST.ctypes.data + 63) & ~63          # host memory, 64-byte aligned


def hp(off=0):
    return C.c_void_p(_BASE + off)


def i64(*v):
    return (C.c_int64 * len(v))(*v)


FN = 'fnn_inflate_segments'
GOOD = (hp(), 64, i64(0, 10, 20), 3, hp(4096), 256, (C.c_uint32 * 1)(), (C.c_int32 * 1)(), None)


def _with(k, v):
    return GOOD[:k] + (v,) + GOOD[k + 1:]


ROWS = [(f'null-{k}', _with(k, None), capi.FNN_E_INVALID, FN + ': NULL argument') for k in (0, 2, 4, 6, 7)] + [
    ('negative-in_bytes', _with(1, -1), capi.FNN_E_INVALID, FN + ': negative size'),
    ('negative-n_starts', _with(3, -1), capi.FNN_E_INVALID, FN + ': negative size'),
    ('negative-out_bytes', _with(5, -1), capi.FNN_E_INVALID, FN + ': negative size'),
    ('in-misaligned', _with(0, hp(8)), capi.FNN_E_INVALID, FN + ': in must be aligned to 16 bytes'),
    ('out-misaligned', _with(4, hp(4100)), capi.FNN_E_INVALID, FN + ': out must be aligned to 16 bytes'),
    ('starts-not-from-0', _with(2, i64(1, 10, 20)), capi.FNN_E_INVALID, FN + ': starts must begin at 0'),
    ('starts-equal', _with(2, i64(0, 10, 10)), capi.FNN_E_INVALID, FN + ': starts must be strictly ascending'),
    ('starts-descending', _with(2, i64(0, 20, 10)), capi.FNN_E_INVALID, FN + ': starts must be strictly ascending'),
    ('starts-reach-in_bytes', _with(2, i64(0, 10, 64)), capi.FNN_E_INVALID, FN + ': every start must lie below in_bytes'),
    ('starts-with-no-input', _with(1, 0), capi.FNN_E_INVALID, FN + ': every start must lie below in_bytes'),
    ('host', GOOD, capi.FNN_E_INVALID, FN + ' needs device pointers for in and out (no CPU path)'),
    ('host-empty', _with(3, 0), capi.FNN_E_INVALID, FN + ' needs device pointers for in and out (no CPU path)'),
]


@pytest.mark.parametrize('row', ROWS, ids=[r[0] for r in ROWS])
def test_refusal_code_and_text(row):
    lib = capi.load_library()
    _, args, code, text = row
    crc, status = GOOD[6], GOOD[7]
    crc[0], status[0] = 0x12345678, 77
    assert (lib.fnn_inflate_segments(*args), lib.fnn_last_error(None).decode()) == (code, text)
    assert (crc[0], status[0]) == (0x12345678, 77), 'a refused call leaves the two host words alone'
