"""The Python model of the speculative device inflate (tests/inflate_any_ref.py) against zlib, on the stream matrix of
tests/inflate_any_cases.py: the model alone inflates every stream of the matrix, which is what makes it fair to ask the same
of ``fnn_inflate_stream`` (tests/test_gpu_inflate_any.py).  No GPU is involved."""
import zlib

import pytest

import inflate_any_cases as cases
import inflate_any_ref as ref


def test_the_matrix_holds_what_the_gpu_tests_rely_on():
    M = cases.matrix()
    assert {int(k.split('-')[1]) for k in M if k.split('-')[0] in ('runs1', 'random')} >= set(cases.SIZES)
    for name, (stream, data) in M.items():
        assert len(data) <= 300000 and zlib.decompress(stream, -15) == data, name
    assert len(cases.small()) >= 40


@pytest.mark.parametrize('kind', cases.KINDS + ('own',))
def test_model_gives_zlibs_bytes_and_crc(kind):
    for name, (stream, data) in cases.matrix().items():
        if name.split('-')[0] != kind:
            continue
        r = ref.inflate(stream, len(data))
        assert r.status == ref.OK, (name, ref.REASONS[r.status])
        assert r.data == data and r.crc == zlib.crc32(data), name
        assert [m[0] for m in r.members] == sorted(set(m[0] for m in r.members)) and set(m[0] for m in r.members) <= set(r.candidates), name


def test_every_true_dynamic_block_start_is_a_candidate():
    """On every stream of at most 8 KiB: a walk of the blocks from bit 0, each block's start where the one before ended, finds
    the non-final dynamic block starts; the finder must hold them all.  Together the streams hold hundreds of them."""
    seen = 0
    for name, (stream, _) in cases.small().items():
        true_starts = ref.dynamic_block_starts(stream)
        assert set(true_starts) <= set(ref.find(stream)), name
        seen += len(true_starts)
    assert seen >= 100, seen


@pytest.mark.parametrize('name', ['runs2-65541-l6-m1', 'runs1-255-l6-m8', 'own-dynamic1-255'])
def test_the_first_test_does_not_change_the_set(name):
    stream = cases.matrix()[name][0]
    assert ref.find(stream) == ref.find_slowly(stream)


def test_hand_made_streams():
    for name, (stream, out_bytes, status, made) in cases.hand_made().items():
        r = ref.inflate(stream, out_bytes)
        assert r.status == status, (name, ref.REASONS[r.status])
        if made is not None:
            assert r.data == made, name
    r = ref.inflate(*cases.hand_made()['marker-through-members'][:2])
    assert len(r.members) == 4 and all(any(e & ref.MARK for e in m[3]) for m in r.members[1:])


def test_coverage_the_gpu_tests_need():
    """From the model's records: a member longer than the ring, runs of members shorter than a window, a member that runs
    through fixed or stored blocks, and 100 cross-member matches in one stream."""
    M = cases.matrix()
    long_one = ref.inflate(*_args(M['runs1-300000-l6-m8']))
    assert max(len(m[3]) for m in long_one.members) > 2 * ref.WINDOW
    short = ref.inflate(*_args(M['ct-300000-l6-m1']))
    assert sum(len(m[3]) < ref.WINDOW for m in short.members) >= 100
    assert len(ref.dynamic_block_starts(M['ct-300000-l6-m1'][0])) < _blocks(M['ct-300000-l6-m1'][0]) - 1
    assert sum(m[5] > 0 for m in short.members) >= 100


def _args(case):
    return case[0], len(case[1])


def _blocks(stream):
    b, n = ref._Bits(bytes(stream), 0), 0
    while True:
        n += 1
        if ref._one_block(stream, b)[0][0]:
            return n


def test_mutated_streams_end_with_a_reason_and_never_with_wrong_bytes():
    seen = set()
    for stream, out_bytes in cases.mutated(300):
        r = ref.inflate(stream, out_bytes)
        seen.add(r.status)
        if r.status == ref.OK:
            d = zlib.decompressobj(-15)
            assert d.decompress(stream) + d.flush() == r.data and d.eof
    assert {ref.OK, ref.END, ref.TABLES, ref.SYMBOL, ref.DISTANCE, ref.FINAL, ref.SIZE, ref.OUTPUT} <= seen, seen


# ---------------------------------------------------------------------- the entries and the switch
import ctypes as C  # noqa: E402
import os  # noqa: E402
import re  # noqa: E402
import struct  # noqa: E402

import numpy as np  # noqa: E402

from fast_nnunet_amd import capi, imageio  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entries_are_declared_exported_and_additive():
    header = open(os.path.join(ROOT, 'include', 'fnn.h')).read()
    lib = capi.load_library()
    for fn in ('fnn_inflate_find_blocks', 'fnn_inflate_stream'):
        assert re.search(r'\b' + fn + r'\s*\(', header) and fn in capi.EXPORTS and hasattr(lib, fn)
    assert '#define FNN_ABI_VERSION 4' in header and lib.fnn_abi_version() == 4
    assert capi.INFLATE_DYN_REASONS == ref.REASONS
    assert 'cannot be inflated in' not in header


_HOST = np.zeros(1 << 14, np.uint8)
_BASE = (_HOST.ctypes.data + 63) & ~63          # host memory, 64-byte aligned


def hp(off=0):
    return C.c_void_p(_BASE + off)


FN = 'fnn_inflate_stream'
GOOD = (hp(), 64, hp(4096), 256, (C.c_uint32 * 1)(), (C.c_int32 * 1)(), None)
FIND = 'fnn_inflate_find_blocks'
GOOD_FIND = (hp(), 64, hp(4096), 4, (C.c_int64 * 1)(), None)


def _with(k, v, good=GOOD):
    return good[:k] + (v,) + good[k + 1:]


ROWS = [(f'null-{k}', FN, _with(k, None), FN + ': NULL argument') for k in (0, 2, 4, 5)] + [
    ('negative-in_bytes', FN, _with(1, -1), FN + ': negative size'),
    ('negative-out_bytes', FN, _with(3, -1), FN + ': negative size'),
    ('in-misaligned', FN, _with(0, hp(8)), FN + ': in must be aligned to 16 bytes'),
    ('out-misaligned', FN, _with(2, hp(4100)), FN + ': out must be aligned to 16 bytes'),
    ('host', FN, GOOD, FN + ' needs device pointers for in and out (no CPU path)'),
    ('host-empty', FN, _with(1, 0), FN + ' needs device pointers for in and out (no CPU path)'),
    ('find-null-in', FIND, _with(0, None, GOOD_FIND), FIND + ': NULL argument'),
    ('find-null-n', FIND, _with(4, None, GOOD_FIND), FIND + ': NULL argument'),
    ('find-null-positions', FIND, _with(2, None, GOOD_FIND), FIND + ': NULL argument'),
    ('find-negative-cap', FIND, _with(3, -1, GOOD_FIND), FIND + ': negative size'),
    ('find-in-misaligned', FIND, _with(0, hp(8), GOOD_FIND), FIND + ': in must be aligned to 16 bytes'),
    ('find-host', FIND, GOOD_FIND, FIND + ' needs a device pointer for in (no CPU path)'),
]


@pytest.mark.parametrize('row', ROWS, ids=[r[0] for r in ROWS])
def test_refusal_code_and_text(row):
    lib = capi.load_library()
    _, fn, args, text = row
    crc, status, n = GOOD[4], GOOD[5], GOOD_FIND[4]
    crc[0], status[0], n[0] = 0x12345678, 77, 55
    assert (getattr(lib, fn)(*args), lib.fnn_last_error(None).decode()) == (capi.FNN_E_INVALID, text)
    assert (crc[0], status[0], n[0]) == (0x12345678, 77, 55), 'a refused call leaves the host words alone'


def test_the_switch_takes_any_as_a_fourth_value():
    for cls in (imageio.NiftiIO, imageio.NiftiReorientIO):
        assert cls(inflate_on_device='any').inflate_on_device == 'any'
        assert cls().inflate_on_device is False and cls(inflate_on_device=True).inflate_on_device is True
        assert cls(inflate_on_device='dynamic').inflate_on_device == 'dynamic'
        for bad in ('Any', 'all', '', 'true'):
            with pytest.raises(ValueError, match='inflate_on_device'):
                cls(inflate_on_device=bad)
    assert imageio.StagedCase([], [], [], 'any').any_stream and not imageio.StagedCase([], [], [], 'dynamic').any_stream


def test_gzip_headers_are_read_per_rfc_1952():
    body = b'\x03\x00' + bytes(8)
    fixed = b'\x1f\x8b\x08%c\x00\x00\x00\x00\x00\x03'
    assert imageio.gzip_member_start(fixed % 0 + body) == 10
    assert imageio.gzip_member_start(fixed % 4 + struct.pack('<H', 5) + b'extra' + body) == 17
    assert imageio.gzip_member_start(fixed % 8 + b'name.nii\x00' + body) == 19
    assert imageio.gzip_member_start(fixed % 16 + b'a comment\x00' + body) == 20
    assert imageio.gzip_member_start(fixed % 2 + b'\x12\x34' + body) == 12
    assert imageio.gzip_member_start(fixed % 30 + struct.pack('<H', 1) + b'x' + b'n\x00' + b'c\x00' + b'\x12\x34' + body) == 10 + 3 + 2 + 2 + 2
    for bad in (fixed % 0x20 + body, fixed % 8 + b'no terminator', fixed % 4 + struct.pack('<H', 500) + body, b'\x1f\x8b\x07' + bytes(30), fixed % 0):
        assert imageio.gzip_member_start(bad) is None
