"""The device inflate that decodes dynamic-Huffman blocks, without a GPU: the Python model of its segment rule and chain
(tests/inflate_dyn_ref.py) against zlib - zlib's own dynamic streams, the project's dynamic fragments, hand-made table
headers (one per rule of csrc/inflate_dyn_core.h), truncated and bit-flipped segments - the entry's declaration, what it
refuses before it touches the device (return code and exact ``fnn_last_error`` text, the rows of tests/test_inflate_cpu.py
under the new name) and the reader's switch."""
import collections
import ctypes as C
import os
import re
import zlib

import numpy as np
import pytest

import inflate_dyn_cases as cases
import inflate_dyn_ref as ref
import inflate_ref
from fast_nnunet_amd import capi, imageio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEG = ref.SEGMENT_MAX


def _block_types(stream: bytes):
    """The BTYPEs of the blocks of a stream that chains, read by following the model segment by segment (a segment's first
    block alone: enough to see that all three kinds occur)."""
    seen, at = collections.Counter(), 0
    while at < len(stream):
        seen[stream[at] >> 1 & 3] += 1
        at = ref.decode_segment(stream, at)[0]
    return seen


# ---------------------------------------------------------------------- the model against zlib
@pytest.mark.parametrize('level', (1, 6, 9))
@pytest.mark.parametrize('k', (100, 4096, SEG))
def test_model_inflates_zlibs_dynamic_full_flush_streams(level, k):
    """The default strategy with Z_FULL_FLUSH every k <= 16384 bytes is a chain of segments under this rule: dynamic blocks,
    on short pieces fixed ones, on random bytes stored ones.  No segment takes more than the input budget."""
    kinds = collections.Counter()
    for name in cases.zlib_data():
        stream, data = cases.zlib_streams()[f'zlib-{name}-l{level}-k{k}']
        assert ref.inflate_raw(stream) == data
        starts = ref.candidates(stream)
        assert ref.chain(stream, starts, len(data)) == (ref.OK, data, zlib.crc32(data)), name
        assert len(starts) >= (len(data) + k - 1) // k
        kinds += _block_types(stream)
        at = 0
        while at < len(stream):
            end = ref.decode_segment(stream, at)[0]
            assert end - at <= 16394 <= ref.INPUT_MAX
            at = end
    assert kinds[2] and kinds[0], kinds
    if k == 100:
        assert kinds[1], kinds


def test_the_fixed_model_refuses_what_this_one_serves():
    stream, data = cases.zlib_streams()['zlib-texty-l6-k4096']
    assert inflate_ref.chain(stream, ref.candidates(stream), len(data))[0] == inflate_ref.DYNAMIC
    assert ref.REASONS == inflate_ref.REASONS + ('TABLES',) and ref.REASONS.index('TABLES') == ref.TABLES == 12


@pytest.mark.parametrize('name', sorted(cases.project_fragments()))
def test_model_inflates_the_projects_dynamic_fragments(name):
    frag, data, n_dynamic = cases.project_fragments()[name]
    starts = ref.candidates(frag)
    assert ref.chain(frag, starts, len(data)) == (ref.OK, data, zlib.crc32(data))
    whole_chunks = [c for c in range(0, len(data), SEG) if len(data) - c >= SEG]
    assert n_dynamic >= len(whole_chunks), 'the chunks of 16384 bytes are dynamic'
    if name in ('fibonacci', 'deep-header'):
        assert n_dynamic == 1 and frag[0] >> 1 & 3 == 2
    dynamic_starts = sum(frag[s] >> 1 & 3 == 2 for s in _chain_starts(frag))
    assert dynamic_starts == n_dynamic


def _chain_starts(stream):
    at, out = 0, []
    while at < len(stream):
        out.append(at)
        at = ref.decode_segment(stream, at)[0]
    return out


@pytest.mark.parametrize('name', sorted(cases.fixed_only_streams()))
def test_fixed_only_streams_give_the_fixed_models_records(name):
    stream, data = cases.fixed_only_streams()[name]
    starts = ref.candidates(stream)
    assert [ref.decode_segment(stream, s) for s in starts] == [inflate_ref.decode_segment(stream, s) for s in starts]
    assert ref.chain(stream, starts, len(data)) == inflate_ref.chain(stream, starts, len(data)) == (ref.OK, data, zlib.crc32(data))


@pytest.mark.parametrize('name', sorted(cases.hand_made()))
def test_hand_made_headers(name):
    """One per rule.  What the model accepts zlib inflates to the same bytes; what it refuses zlib refuses."""
    stream, reason, made = cases.hand_made()[name]
    end, out, got = ref.decode_segment(stream, 0)
    assert ref.REASONS[got] == ref.REASONS[reason]
    if reason == ref.OK:
        assert out == made and end == len(stream) and cases.zlib_says(stream) == made
    else:
        assert end == -1 and cases.zlib_says(stream) is None


def test_the_rule_is_zlibs():
    """4000 truncated and bit-flipped segments: where the model says OK, zlib gives the same bytes and reaches the end; where
    it says TABLES, SYMBOL, DISTANCE, NLEN or BTYPE3, zlib raises."""
    seen = collections.Counter()
    for case, s in enumerate(cases.mutated(4000)):
        end, out, reason = ref.decode_segment(s, 0)
        seen[ref.REASONS[reason]] += 1
        if reason == ref.OK:
            assert cases.zlib_says(s[:end]) == out, case
        elif reason in (ref.TABLES, ref.SYMBOL, ref.DISTANCE, ref.NLEN, ref.BTYPE3):
            assert cases.zlib_says(s) is None, (case, ref.REASONS[reason])
    assert seen['DYNAMIC'] == 0 and min(seen[r] for r in ('OK', 'TABLES', 'SYMBOL', 'DISTANCE', 'NLEN', 'END')) > 0, seen
    assert seen['TABLES'] > 400, seen


# ---------------------------------------------------------------------- the entry
def test_entry_is_declared_exported_and_additive():
    header = open(os.path.join(ROOT, 'include', 'fnn.h')).read()
    lib = capi.load_library()
    assert re.search(r'\bfnn_inflate_segments_dyn\s*\(', header) and 'fnn_inflate_segments_dyn' in capi.EXPORTS and hasattr(lib, 'fnn_inflate_segments_dyn')
    assert '#define FNN_ABI_VERSION 4' in header and lib.fnn_abi_version() == 4
    assert re.search(r'#define FNN_INFLATE_TABLES 12\b', header) and capi.FNN_INFLATE_TABLES == 12
    assert capi.INFLATE_REASONS == inflate_ref.REASONS and len(capi.INFLATE_REASONS) == 12
    assert capi.INFLATE_DYN_REASONS == ref.REASONS


_HOST = np.zeros(1 << 14, np.uint8)
_BASE = (_HOST.ctypes.data + 63) & ~63          # host memory, 64-byte aligned


def hp(off=0):
    return C.c_void_p(_BASE + off)


def i64(*v):
    return (C.c_int64 * len(v))(*v)


FN = 'fnn_inflate_segments_dyn'
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
    assert (lib.fnn_inflate_segments_dyn(*args), lib.fnn_last_error(None).decode()) == (code, text)
    assert (crc[0], status[0]) == (0x12345678, 77), 'a refused call leaves the two host words alone'


# ---------------------------------------------------------------------- the switch
def test_the_switch_takes_false_true_and_dynamic():
    for cls in (imageio.NiftiIO, imageio.NiftiReorientIO):
        assert cls().inflate_on_device is False
        assert cls(inflate_on_device=True).inflate_on_device is True
        assert cls(inflate_on_device=False).inflate_on_device is False
        assert cls(inflate_on_device='dynamic').inflate_on_device == 'dynamic'
        assert cls(inflate_on_device=1).inflate_on_device is True and cls(inflate_on_device=None).inflate_on_device is False
        for bad in ('Dynamic', 'fixed', '', 'true'):
            with pytest.raises(ValueError, match='inflate_on_device'):
                cls(inflate_on_device=bad)
    assert imageio.StagedCase([], [], [], 'dynamic').inflate_on_device is True
