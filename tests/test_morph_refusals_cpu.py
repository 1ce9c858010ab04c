"""fnn_binary_morphology's refusals through the library with null device pointers: every one of them returns before any launch
and before any device memory is asked for, so none needs a GPU.  Also: the symbol is exported, declared and bound, and the
ABI version is still 4."""
import ctypes as C
import os
import re

from fast_nnunet_amd import capi

FN = 'fnn_binary_morphology'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _entry_text(*args):
    lib = capi.load_library()
    code = getattr(lib, FN)(*args)
    return code, lib.fnn_last_error(None).decode()


def test_symbol_is_exported_and_the_abi_version_stays_4():
    lib = capi.load_library()
    header = open(os.path.join(ROOT, 'include', 'fnn.h')).read()
    assert re.search(r'\b' + FN + r'\s*\(', header) and FN in capi.EXPORTS and hasattr(lib, FN)
    assert lib.fnn_abi_version() == 4
    m = re.search(r'enum \{ FNN_MORPH_DILATE = 0, FNN_MORPH_ERODE = 1, FNN_MORPH_OPEN = 2, FNN_MORPH_CLOSE = 3 \};', header)
    assert m and (capi.FNN_MORPH_DILATE, capi.FNN_MORPH_ERODE, capi.FNN_MORPH_OPEN, capi.FNN_MORPH_CLOSE) == (0, 1, 2, 3)


def test_the_entry_refuses_bad_arguments_without_a_gpu():
    shape, member = (C.c_int64 * 3)(2, 2, 2), (C.c_int32 * 3)(-1, 0, -1)
    buf = (C.c_uint8 * 8)()
    U8, U16 = capi.FNN_LABEL_U8, capi.FNN_LABEL_U16
    #       0    1   2      3       4  5 op                 6 conn 7 n 8 border 9 bg 10 fill 11 axes 12 changed 13 stream
    good = [buf, U8, shape, member, 3, capi.FNN_MORPH_CLOSE, 6, 1, 0, 0, 1, 7, None, None]

    def bad(i, v, base=None):
        base = good if base is None else base
        return base[:i] + [v] + base[i + 1:]
    INV, UNS = capi.FNN_E_INVALID, capi.FNN_E_UNSUPPORTED
    assert _entry_text(*bad(2, None)) == (INV, 'NULL shape')
    assert _entry_text(*bad(1, 7)) == (INV, 'unknown label dtype')
    for op in (-1, 4, 100):
        assert _entry_text(*bad(5, op)) == (INV, 'op must be FNN_MORPH_DILATE, ERODE, OPEN or CLOSE (0..3)')
    for conn in (0, 1, 3, 8, 27, -6):
        assert _entry_text(*bad(6, conn)) == (INV, 'connectivity must be 6, 18 or 26')
    for n in (0, -1, 1025, 2 ** 31 - 1):
        assert _entry_text(*bad(7, n)) == (INV, 'iterations must be 1..1024')
    for b in (2, -1):
        assert _entry_text(*bad(8, b)) == (INV, 'border_value must be 0 or 1')
    assert _entry_text(*bad(9, 256)) == (INV, 'background_label outside the label dtype')
    assert _entry_text(*bad(9, -1)) == (INV, 'background_label outside the label dtype')
    assert _entry_text(*bad(9, 65536, bad(1, U16))) == (INV, 'background_label outside the label dtype')
    assert _entry_text(*bad(10, 256)) == (INV, 'fill_label outside the label dtype')
    assert _entry_text(*bad(10, -1)) == (INV, 'fill_label outside the label dtype')
    for op in (capi.FNN_MORPH_DILATE, capi.FNN_MORPH_CLOSE):                       # the adding ops need a fill label of their own
        assert _entry_text(*bad(10, 0, bad(5, op))) == (INV, 'fill_label equals background_label')
    for axes in (0, 8, -1):
        assert _entry_text(*bad(11, axes)) == (INV, 'axes must be 1..7 (bit a: the structure spans axis a)')
    assert _entry_text(*bad(2, (C.c_int64 * 3)(2, -1, 2))) == (INV, 'negative shape')
    assert _entry_text(*bad(3, None)) == (INV, 'bad label-set table')
    assert _entry_text(*bad(4, -1)) == (INV, 'bad label-set table')
    for entry in (1, -2):
        assert _entry_text(*bad(3, (C.c_int32 * 3)(-1, entry, -1))) == (INV, 'group_of_label entry outside [-1, 0]')
    assert _entry_text(*bad(2, (C.c_int64 * 3)(2048, 2048, 1024))) == (UNS, FN + ': more than 2^31 - 1 voxels')
    assert _entry_text(*bad(2, (C.c_int64 * 3)(2 ** 31, 1, 1))) == (UNS, FN + ': more than 2^31 - 1 voxels')
    # everything in order: the refusal is the missing device map, for every op, connectivity and border value
    for op in range(4):
        for conn in (6, 18, 26):
            for b in (0, 1):
                args = bad(8, b, bad(6, conn, bad(5, op)))
                assert _entry_text(*args) == (INV, FN + ' needs a device label map (no CPU path)')
                assert _entry_text(*bad(0, None, args)) == (INV, FN + ' needs a device label map (no CPU path)')
    # erosion and opening do not read fill_label
    for op in (capi.FNN_MORPH_ERODE, capi.FNN_MORPH_OPEN):
        for fill in (0, -5, 70000):
            assert _entry_text(*bad(10, fill, bad(5, op))) == (INV, FN + ' needs a device label map (no CPU path)')
    assert _entry_text(*bad(7, 1024)) == (INV, FN + ' needs a device label map (no CPU path)')


def test_a_zero_size_volume_returns_0_and_a_zero_count():
    member = (C.c_int32 * 3)(-1, 0, -1)
    lib = capi.load_library()
    for zero in ((0, 4, 4), (4, 0, 4), (4, 4, 0)):
        changed = C.c_int64(9)
        assert getattr(lib, FN)(None, capi.FNN_LABEL_U8, (C.c_int64 * 3)(*zero), member, 3, capi.FNN_MORPH_DILATE, 26, 3, 1, 0, 1, 7,
                                C.byref(changed), None) == 0
        assert changed.value == 0
