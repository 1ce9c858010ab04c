"""What fnn_surface_count and fnn_surface_distances refuse before they touch the device: bad calls through the C ABI with
the return code and the exact fnn_last_error(NULL) text of each, in the manner of tests/test_entry_refusals_cpu.py.  No
machine without a GPU owns device memory, so every call ends at the latest at the device-pointer refusal."""
import ctypes as C
import math

import numpy as np
import pytest

from fast_nnunet_amd import capi

INVALID, UNSUPPORTED = capi.FNN_E_INVALID, capi.FNN_E_UNSUPPORTED
U8, U16 = capi.FNN_LABEL_U8, capi.FNN_LABEL_U16

_HOST = np.zeros(1 << 14, np.uint8)
_BASE = (_HOST.ctypes.data + 63) & ~63          # host memory, 64-byte aligned


def hp(off=0):
    return C.c_void_p(_BASE + off)


def i64(*v):
    return (C.c_int64 * len(v))(*v)


def f64(*v):
    return (C.c_double * len(v))(*v)


def u8(*v):
    return (C.c_uint8 * len(v))(*v)


NULL = None
S3, MEMBER, SPACING = i64(4, 4, 4), u8(0, 1, 0, 0, 0, 1), f64(1.0, 1.0, 1.0)
N_SURFACE, BOXES = i64(*[0] * 4), i64(*[0] * 12)
COUNT, DIST = 'fnn_surface_count', 'fnn_surface_distances'
#        ref   pred      dtype shape member n_table n_regions ...
GOOD = {COUNT: (hp(), hp(4096), U8, S3, MEMBER, 3, 2, N_SURFACE, BOXES, NULL),
        DIST: (hp(), hp(4096), U8, S3, MEMBER, 3, 2, SPACING, hp(8192), 64, NULL)}
DEVMSG = {COUNT: COUNT + ' needs device label maps (no CPU path)',
          DIST: DIST + ' needs device pointers for ref, pred and sq_dist (no CPU path)'}


def _with(args, k, v):
    return args[:k] + (v,) + args[k + 1:]


def _rows():
    R = []
    for fn, g in GOOD.items():
        nulls = (3, 4, 7, 8) if fn == COUNT else (3, 4, 7)
        R += [(f'{fn}-null-{k}', fn, _with(g, k, NULL), INVALID, fn + ': NULL argument') for k in nulls]
        R += [(f'{fn}-null-map-{k}', fn, _with(g, k, NULL), INVALID, DEVMSG[fn]) for k in (0, 1)]
        R += [(fn + '-host', fn, g, INVALID, DEVMSG[fn]),
              (fn + '-host-u16', fn, _with(g, 2, U16), INVALID, DEVMSG[fn]),
              (fn + '-dtype', fn, _with(g, 2, 2), INVALID, 'unknown label dtype'),
              (fn + '-dtype-negative', fn, _with(g, 2, -1), INVALID, 'unknown label dtype'),
              (fn + '-regions0', fn, _with(g, 6, 0), INVALID, fn + ': n_regions must be 1..1024'),
              (fn + '-regions-negative', fn, _with(g, 6, -3), INVALID, fn + ': n_regions must be 1..1024'),
              (fn + '-regions1025', fn, _with(g, 6, 1025), INVALID, fn + ': n_regions must be 1..1024'),
              (fn + '-negative-table', fn, _with(g, 5, -1), INVALID, fn + ': negative n_table'),
              (fn + '-negative-extent', fn, _with(g, 3, i64(4, -1, 4)), INVALID, fn + ': negative extent'),
              (fn + '-too-large', fn, _with(g, 3, i64(2048, 2048, 512)), UNSUPPORTED, fn + ': more than 2^31 - 1 voxels'),
              (fn + '-overflow', fn, _with(g, 3, i64(1 << 31, 1 << 31, 1 << 31)), UNSUPPORTED, fn + ': more than 2^31 - 1 voxels'),
              (fn + '-misaligned-u16', fn, _with(_with(g, 2, U16), 1, hp(4097)), INVALID, fn + ': label maps must be aligned to their element')]
    g = GOOD[DIST]
    for name, bad in {'zero': 0.0, 'negative': -1.0, 'nan': math.nan, 'inf': math.inf}.items():
        for k in range(3):
            sp = [1.0, 2.0, 0.5]
            sp[k] = bad
            R.append((f'{DIST}-spacing-{name}-{k}', DIST, _with(g, 7, f64(*sp)), INVALID, DIST + ': spacing must be finite and positive'))
    R += [(DIST + '-negative-cap', DIST, _with(g, 9, -1), INVALID, DIST + ': cap is negative'),
          (DIST + '-null-sq_dist', DIST, _with(g, 8, NULL), INVALID, DEVMSG[DIST]),
          (DIST + '-misaligned-sq_dist', DIST, _with(g, 8, hp(8196)), INVALID, DIST + ': sq_dist must be 8-byte aligned')]
    return R


ROWS = _rows()


def call(row):
    _, fn, args, _, _ = row
    lib = capi.load_library()
    code = getattr(lib, fn)(*args)
    return code, lib.fnn_last_error(None).decode()


@pytest.mark.parametrize('row', ROWS, ids=[r[0] for r in ROWS])
def test_refusal_code_and_text(row):
    assert call(row) == (row[3], row[4])


def test_the_entries_are_declared_exported_and_additive():
    lib = capi.load_library()
    assert lib.fnn_abi_version() == 4
    for fn in (COUNT, DIST):
        assert fn in capi.EXPORTS and hasattr(lib, fn)
    assert len({r[0] for r in ROWS}) == len(ROWS)


def test_a_volume_without_voxels_is_zeros_and_no_launch():
    lib = capi.load_library()
    n_surface, boxes = i64(*[7] * 4), i64(*[7] * 12)
    assert lib.fnn_surface_count(hp(), hp(4096), U8, i64(4, 0, 4), MEMBER, 3, 2, n_surface, boxes, NULL) == 0
    assert list(n_surface) == [0] * 4 and list(boxes) == [0] * 12
    assert lib.fnn_surface_distances(hp(), hp(4096), U8, i64(0, 4, 4), MEMBER, 3, 2, SPACING, hp(8192), 0, NULL) == 0
