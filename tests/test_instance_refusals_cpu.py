"""What fnn_instance_overlaps refuses before it touches the device: bad calls through the C ABI with the return code and the
exact fnn_last_error(NULL) text of each, in the manner of tests/test_surface_refusals_cpu.py.  No machine without a GPU owns
device memory, so every call ends at the latest at the device-pointer refusal."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from fast_nnunet_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED = capi.FNN_E_INVALID, capi.FNN_E_UNSUPPORTED
U8, U16 = capi.FNN_LABEL_U8, capi.FNN_LABEL_U16
FN = 'fnn_instance_overlaps'

_HOST = np.zeros(1 << 14, np.uint8)
_BASE = (_HOST.ctypes.data + 63) & ~63          # host memory, 64-byte aligned


def hp(off=0):
    return C.c_void_p(_BASE + off)


def i64(*v):
    return (C.c_int64 * len(v))(*v)


def i32(*v):
    return (C.c_int32 * len(v))(*v)


NULL = None
S3, TABLE, N_OUT = i64(4, 4, 4), i32(-1, 0, 1), i64(7, 7, 7)
#       ref   pred      dtype shape table n_table n_groups records cap n_out stream
GOOD = (hp(), hp(4096), U8, S3, TABLE, 3, 2, hp(8192), 64, N_OUT, NULL)
DEVMSG = FN + ' needs device pointers for ref, pred and records (no CPU path)'


def _with(args, k, v):
    return args[:k] + (v,) + args[k + 1:]


ROWS = [(f'null-{k}', _with(GOOD, k, NULL), INVALID, FN + ': NULL argument') for k in (3, 4, 9)]
ROWS += [(f'null-pointer-{k}', _with(GOOD, k, NULL), INVALID, DEVMSG) for k in (0, 1, 7)]
ROWS += [('host', GOOD, INVALID, DEVMSG),
         ('host-u16', _with(GOOD, 2, U16), INVALID, DEVMSG),
         ('dtype', _with(GOOD, 2, 2), INVALID, 'unknown label dtype'),
         ('dtype-negative', _with(GOOD, 2, -1), INVALID, 'unknown label dtype'),
         ('groups0', _with(GOOD, 6, 0), INVALID, FN + ': n_groups must be 1..1024'),
         ('groups-negative', _with(GOOD, 6, -3), INVALID, FN + ': n_groups must be 1..1024'),
         ('groups1025', _with(GOOD, 6, 1025), INVALID, FN + ': n_groups must be 1..1024'),
         ('negative-table', _with(GOOD, 5, -1), INVALID, FN + ': negative n_table'),
         ('entry-too-large', _with(GOOD, 4, i32(-1, 0, 2)), INVALID, FN + ': group_of_label entry outside [-1, n_groups)'),
         ('entry-too-small', _with(GOOD, 4, i32(-2, 0, 1)), INVALID, FN + ': group_of_label entry outside [-1, n_groups)'),
         ('negative-extent', _with(GOOD, 3, i64(4, -1, 4)), INVALID, FN + ': negative extent'),
         ('negative-cap', _with(GOOD, 8, -1), INVALID, FN + ': cap is negative'),
         ('too-large', _with(GOOD, 3, i64(2048, 2048, 512)), UNSUPPORTED, FN + ': more than 2^31 - 1 voxels'),
         ('overflow', _with(GOOD, 3, i64(1 << 31, 1 << 31, 1 << 31)), UNSUPPORTED, FN + ': more than 2^31 - 1 voxels'),
         ('misaligned-u16', _with(_with(GOOD, 2, U16), 1, hp(4097)), INVALID, FN + ': label maps must be aligned to their element'),
         ('misaligned-records', _with(GOOD, 7, hp(8194)), INVALID, FN + ': records must be 4-byte aligned'),
         ('empty-table-host', _with(_with(GOOD, 4, NULL), 5, 0), INVALID, DEVMSG)]


def call(args):
    lib = capi.load_library()
    code = getattr(lib, FN)(*args)
    return code, lib.fnn_last_error(None).decode()


@pytest.mark.parametrize('row', ROWS, ids=[r[0] for r in ROWS])
def test_refusal_code_and_text(row):
    assert call(row[1]) == (row[2], row[3])


def test_the_entry_is_declared_exported_and_additive():
    lib = capi.load_library()
    assert lib.fnn_abi_version() == 4
    assert FN in capi.EXPORTS and hasattr(lib, FN)
    header = open(os.path.join(ROOT, 'include', 'fnn.h')).read()
    assert re.search(r'\bint\s+' + FN + r'\s*\(', header)
    assert capi.INSTANCE_FIRST_CAPACITY == 65536
    assert len({r[0] for r in ROWS}) == len(ROWS)


def test_a_volume_without_voxels_is_zeros_and_no_launch():
    lib = capi.load_library()
    for shape in (i64(4, 0, 4), i64(0, 4, 4), i64(4, 4, 0)):
        n_out = i64(7, 7, 7)
        assert getattr(lib, FN)(hp(), hp(4096), U8, shape, TABLE, 3, 2, hp(8192), 0, n_out, NULL) == 0
        assert list(n_out) == [0, 0, 0]
