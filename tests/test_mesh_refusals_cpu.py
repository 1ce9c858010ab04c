"""What fnn_mesh_count, fnn_mesh_emit and fast_nnunet_amd.meshing refuse before they touch the device: bad calls through
the C ABI with the return code and the exact fnn_last_error(NULL) text of each, in the manner of
tests/test_surface_refusals_cpu.py, and every refusal of the Python layer.  No machine without a GPU owns device memory, so
every C call ends at the latest at the device-pointer refusal."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from fast_nnunet_amd import capi, meshing

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
S3, MEMBER = i64(4, 4, 4), u8(0, 1, 0, 0, 0, 1)
EYE = [1.0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1]
COUNTS, BOXES = i64(*[0] * 4), i64(*[0] * 12)
COUNT, EMIT = 'fnn_mesh_count', 'fnn_mesh_emit'
#        seg  dtype shape member n_table n_regions ...
GOOD = {COUNT: (hp(), U8, S3, MEMBER, 3, 2, COUNTS, BOXES, NULL),
        #                                          affine  pairs layout points cap cells cap region stream
        EMIT: (hp(), U8, S3, MEMBER, 3, 2, f64(*EYE), 1, 0, hp(4096), 64, hp(8192), 64, hp(12288), NULL)}
DEVMSG = {COUNT: COUNT + ' needs a device label map (no CPU path)',
          EMIT: EMIT + ' needs device pointers for seg, points, cells and cell_region (no CPU path)'}


def _with(args, k, v):
    return args[:k] + (v,) + args[k + 1:]


def _rows():
    R = []
    for fn, g in GOOD.items():
        nulls = (2, 3, 6, 7) if fn == COUNT else (2, 3, 6)
        R += [(f'{fn}-null-{k}', fn, _with(g, k, NULL), INVALID, fn + ': NULL argument') for k in nulls]
        R += [(fn + '-null-map', fn, _with(g, 0, NULL), INVALID, DEVMSG[fn]),
              (fn + '-host', fn, g, INVALID, DEVMSG[fn]),
              (fn + '-host-u16', fn, _with(g, 1, U16), INVALID, DEVMSG[fn]),
              (fn + '-dtype', fn, _with(g, 1, 2), INVALID, 'unknown label dtype'),
              (fn + '-dtype-negative', fn, _with(g, 1, -1), INVALID, 'unknown label dtype'),
              (fn + '-regions0', fn, _with(g, 5, 0), INVALID, fn + ': n_regions must be 1..1024'),
              (fn + '-regions-negative', fn, _with(g, 5, -3), INVALID, fn + ': n_regions must be 1..1024'),
              (fn + '-regions1025', fn, _with(g, 5, 1025), INVALID, fn + ': n_regions must be 1..1024'),
              (fn + '-negative-table', fn, _with(g, 4, -1), INVALID, fn + ': negative n_table'),
              (fn + '-negative-extent', fn, _with(g, 2, i64(4, -1, 4)), INVALID, fn + ': negative extent'),
              (fn + '-too-large', fn, _with(g, 2, i64(2048, 2048, 512)), UNSUPPORTED, fn + ': more than 2^31 - 1 voxels'),
              (fn + '-overflow', fn, _with(g, 2, i64(1 << 31, 1 << 31, 1 << 31)), UNSUPPORTED, fn + ': more than 2^31 - 1 voxels'),
              (fn + '-misaligned-u16', fn, _with(_with(g, 1, U16), 0, hp(1)), INVALID, fn + ': the label map must be aligned to its element')]
    g = GOOD[EMIT]
    for name, bad in {'nan': math.nan, 'inf': math.inf, '-inf': -math.inf}.items():
        for k in (0, 7, 15):
            a = list(EYE)
            a[k] = bad
            R.append((f'{EMIT}-affine-{name}-{k}', EMIT, _with(g, 6, f64(*a)), INVALID, EMIT + ': the affine must be finite'))
    align0 = EMIT + ': points must be 4-byte, cells 4-byte and cell_region 2-byte aligned'
    align1 = EMIT + ': points must be 4-byte, cells 16-byte and cell_region 2-byte aligned'
    R += [(EMIT + '-negative-pairs', EMIT, _with(g, 7, -1), INVALID, EMIT + ': smoothing_pairs is negative'),
          (EMIT + '-layout2', EMIT, _with(g, 8, 2), INVALID, EMIT + ': unknown layout'),
          (EMIT + '-layout-negative', EMIT, _with(g, 8, -1), INVALID, EMIT + ': unknown layout'),
          (EMIT + '-negative-cap-points', EMIT, _with(g, 10, -1), INVALID, EMIT + ': a cap is negative'),
          (EMIT + '-negative-cap-cells', EMIT, _with(g, 12, -1), INVALID, EMIT + ': a cap is negative'),
          (EMIT + '-misaligned-points', EMIT, _with(g, 9, hp(4098)), INVALID, align0),
          (EMIT + '-misaligned-cells', EMIT, _with(g, 11, hp(8194)), INVALID, align0),
          (EMIT + '-misaligned-cells-vtk', EMIT, _with(_with(g, 8, 1), 11, hp(8196)), INVALID, align1),
          (EMIT + '-misaligned-region', EMIT, _with(g, 13, hp(12289)), INVALID, align0),
          (EMIT + '-null-points', EMIT, _with(g, 9, NULL), INVALID, DEVMSG[EMIT]),
          (EMIT + '-null-cells', EMIT, _with(g, 11, NULL), INVALID, DEVMSG[EMIT]),
          (EMIT + '-null-region', EMIT, _with(g, 13, NULL), INVALID, DEVMSG[EMIT]),
          (EMIT + '-host-vtk', EMIT, _with(g, 8, 1), INVALID, DEVMSG[EMIT])]
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
    for fn in (COUNT, EMIT):
        assert fn in capi.EXPORTS and hasattr(lib, fn)
    assert len({r[0] for r in ROWS}) == len(ROWS)


def test_a_volume_without_voxels_is_zeros_and_no_launch():
    lib = capi.load_library()
    counts, boxes = i64(*[7] * 4), i64(*[7] * 12)
    assert lib.fnn_mesh_count(hp(), U8, i64(4, 0, 4), MEMBER, 3, 2, counts, boxes, NULL) == 0
    assert list(counts) == [0] * 4 and list(boxes) == [0] * 12
    assert lib.fnn_mesh_emit(*_with(GOOD[EMIT], 2, i64(0, 4, 4))) == 0
    before = _HOST.copy()
    assert lib.fnn_mesh_emit(*_with(_with(GOOD[EMIT], 2, i64(4, 4, 0)), 8, 1)) == 0
    assert np.array_equal(_HOST, before)


# ---- the Python layer: every refusal comes before any GPU call (none of these needs a GPU)
SEG = np.zeros((3, 4, 5), np.uint8)
BAD_CALLS = {
    'float-map': (dict(seg=np.zeros((3, 4, 5), np.float32)), ValueError, 'integer dtype'),
    'bool-map': (dict(seg=np.zeros((3, 4, 5), bool)), ValueError, 'integer dtype'),
    'float-tensor': (dict(seg=torch.zeros(3, 4, 5)), ValueError, 'integer dtype'),
    '2d-map': (dict(seg=np.zeros((4, 5), np.uint8)), ValueError, '3-D'),
    '4d-map': (dict(seg=np.zeros((1, 3, 4, 5), np.uint8)), ValueError, '3-D'),
    'negative-value': (dict(seg=np.full((3, 4, 5), -1, np.int32)), ValueError, '0..65535'),
    'large-value': (dict(seg=np.full((3, 4, 5), 65536, np.int32)), ValueError, '0..65535'),
    'negative-label': (dict(seg=SEG, labels_or_regions=[1, -2]), ValueError, 'label -2 is outside 0..65535'),
    'large-label': (dict(seg=SEG, labels_or_regions=[(1, 65536)]), ValueError, 'label 65536 is outside 0..65535'),
    'empty-region': (dict(seg=SEG, labels_or_regions=[()]), ValueError, 'without label ids'),
    'too-many-regions': (dict(seg=SEG, labels_or_regions=list(range(1, 1026))), ValueError, 'at most 1024'),
    'smoothing-negative': (dict(seg=SEG, smoothing_factor=-0.01), ValueError, 'smoothing_factor'),
    'smoothing-above-one': (dict(seg=SEG, smoothing_factor=1.01), ValueError, 'smoothing_factor'),
    'smoothing-nan': (dict(seg=SEG, smoothing_factor=math.nan), ValueError, 'smoothing_factor'),
    'affine-and-spacing': (dict(seg=SEG, affine=np.eye(4), spacing=(1, 1, 1)), ValueError, 'not both'),
    'affine-3x3': (dict(seg=SEG, affine=np.eye(3)), ValueError, '4x4'),
    'affine-nan': (dict(seg=SEG, affine=np.diag([1, math.nan, 1, 1])), ValueError, 'finite'),
    'affine-singular': (dict(seg=SEG, affine=np.diag([1.0, 0, 1, 1])), ValueError, 'invertible'),
    'spacing-zero': (dict(seg=SEG, spacing=(1, 0, 1)), ValueError, 'spacing'),
    'spacing-two': (dict(seg=SEG, spacing=(1, 1)), ValueError, 'spacing'),
    'coordinate-system': (dict(seg=SEG, coordinate_system='RAI'), ValueError, 'coordinate_system'),
}


@pytest.fixture
def no_gpu_call(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError('a GPU call was made before the refusal')
    for name in ('mesh_count', 'mesh_emit'):
        monkeypatch.setattr(capi, name, refuse)
    monkeypatch.setattr(meshing, '_device', refuse)
    monkeypatch.setattr(meshing, '_to_device', refuse)


@pytest.mark.parametrize('name', list(BAD_CALLS))
def test_label_surfaces_refuses_before_any_gpu_call(name, no_gpu_call):
    kwargs, error, text = BAD_CALLS[name]
    with pytest.raises(error, match=text):
        meshing.label_surfaces(**kwargs)


def test_the_generator_refuses_decimation_and_bad_smoothing(no_gpu_call, tmp_path):
    gen = meshing.VTKModelGenerator()
    out = str(tmp_path / 'm.vtk')
    for call_ in (lambda **k: gen.generate_vtk_model('mask.nii.gz', out, **k), lambda **k: gen.generate_from_labels(SEG, {}, out, **k)):
        with pytest.raises(NotImplementedError, match='decimation_factor'):
            call_(decimation_factor=0.2)
        with pytest.raises(ValueError, match='smoothing_factor'):
            call_(smoothing_factor=1.5)
    with pytest.raises(ValueError, match='coordinate_system'):
        gen.generate_vtk_model('mask.nii.gz', out, coordinate_system='xyz')
    assert meshing.smoothing_pairs(0.5) == 25 and meshing.PAIRS_AT_FACTOR_ONE == 50
    with pytest.raises(FileNotFoundError):
        meshing.VTKModelGenerator(color_file_path=str(tmp_path / 'missing.txt'))
