"""What fnn_mesh_decimate and the decimation arguments of fast_nnunet_amd.meshing refuse before they touch the device: bad
calls through the C ABI with the return code and the exact fnn_last_error(NULL) text of each, in the manner of
tests/test_mesh_refusals_cpu.py, and every refusal of the Python layer.  No machine without a GPU owns device memory, so
every C call ends at the latest at the device-pointer refusal."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from fast_nnunet_amd import capi, meshing

INVALID, UNSUPPORTED = capi.FNN_E_INVALID, capi.FNN_E_UNSUPPORTED
FN = 'fnn_mesh_decimate'

_HOST = np.zeros(1 << 14, np.uint8)
_BASE = (_HOST.ctypes.data + 63) & ~63          # host memory, 64-byte aligned


def hp(off=0):
    return C.c_void_p(_BASE + off)


def i64(*v):
    return (C.c_int64 * len(v))(*v)


NULL = None
COUNTS, STATUS = i64(*[7] * 4), i64(*[7] * 4)
#       points n  cells     region    t  offsets   R  factor layout out_points cap out_cells cap out_region counts status stream
GOOD = (hp(), 8, hp(2048), hp(4096), 4, i64(0, 8), 1, 0.5, 0, hp(6144), 8, hp(8192), 4, hp(10240), COUNTS, STATUS, NULL)
DEVMSG = FN + ' needs device pointers for the model and the result (no CPU path)'
ALIGN_IN = FN + ': points and cells must be 4-byte and cell_region 2-byte aligned'
ALIGN0 = FN + ': out_points must be 4-byte, out_cells 4-byte and out_cell_region 2-byte aligned'
ALIGN1 = FN + ': out_points must be 4-byte, out_cells 16-byte and out_cell_region 2-byte aligned'


def _with(args, *pairs):
    args = list(args)
    for k, v in zip(pairs[::2], pairs[1::2]):
        args[k] = v
    return tuple(args)


def _rows():
    g = GOOD
    R = [(f'null-{k}', _with(g, k, NULL), INVALID, FN + ': NULL argument') for k in (5, 14, 15)]
    R += [(f'null-device-{k}', _with(g, k, NULL), INVALID, DEVMSG) for k in (0, 2, 3, 9, 11, 13)]
    R += [('host', g, INVALID, DEVMSG), ('host-vtk', _with(g, 8, 1), INVALID, DEVMSG),
          ('negative-n', _with(g, 1, -1), INVALID, FN + ': a count is negative'),
          ('negative-t', _with(g, 4, -1), INVALID, FN + ': a count is negative'),
          ('regions-negative', _with(g, 6, -1), INVALID, FN + ': n_regions must be 0..1024'),
          ('regions1025', _with(g, 6, 1025), INVALID, FN + ': n_regions must be 0..1024'),
          ('layout2', _with(g, 8, 2), INVALID, FN + ': unknown layout'),
          ('layout-negative', _with(g, 8, -1), INVALID, FN + ': unknown layout'),
          ('negative-cap-points', _with(g, 10, -1), INVALID, FN + ': a cap is negative'),
          ('negative-cap-cells', _with(g, 12, -1), INVALID, FN + ': a cap is negative'),
          ('offsets-short', _with(g, 5, i64(0, 7)), INVALID, FN + ': point_offsets must rise from 0 to n'),
          ('offsets-long', _with(g, 5, i64(0, 9)), INVALID, FN + ': point_offsets must rise from 0 to n'),
          ('offsets-from-one', _with(g, 5, i64(1, 8)), INVALID, FN + ': point_offsets must rise from 0 to n'),
          ('offsets-falling', _with(g, 5, i64(0, 9, 8), 6, 2), INVALID, FN + ': point_offsets must rise from 0 to n'),
          ('no-region', _with(g, 1, 0, 5, i64(0), 6, 0), INVALID, FN + ': triangles without a region'),
          ('too-many-points', _with(g, 1, 1 << 31, 5, i64(0, 1 << 31)), UNSUPPORTED, FN + ': more than 2^31 - 1 points or triangle corners'),
          ('too-many-corners', _with(g, 4, (2 ** 31 - 1) // 3 + 1), UNSUPPORTED, FN + ': more than 2^31 - 1 points or triangle corners'),
          ('misaligned-points', _with(g, 0, hp(2)), INVALID, ALIGN_IN),
          ('misaligned-cells', _with(g, 2, hp(2050)), INVALID, ALIGN_IN),
          ('misaligned-region', _with(g, 3, hp(4097)), INVALID, ALIGN_IN),
          ('misaligned-out-points', _with(g, 9, hp(6146)), INVALID, ALIGN0),
          ('misaligned-out-cells', _with(g, 11, hp(8194)), INVALID, ALIGN0),
          ('misaligned-out-cells-vtk', _with(g, 8, 1, 11, hp(8196)), INVALID, ALIGN1),
          ('misaligned-out-region', _with(g, 13, hp(10241)), INVALID, ALIGN0)]
    for name, bad in {'one': 1.0, 'above-one': 1.5, 'negative': -0.01, 'nan': math.nan, 'inf': math.inf, '-inf': -math.inf}.items():
        R.append(('factor-' + name, _with(g, 7, bad), INVALID, FN + ': decimation_factor must lie in [0, 1)'))
    return R


ROWS = _rows()


@pytest.mark.parametrize('row', ROWS, ids=[r[0] for r in ROWS])
def test_refusal_code_and_text(row):
    lib = capi.load_library()
    code = lib.fnn_mesh_decimate(*row[1])
    assert (code, lib.fnn_last_error(None).decode()) == (row[2], row[3])


def test_the_entry_is_declared_exported_and_additive():
    lib = capi.load_library()
    assert lib.fnn_abi_version() == 4
    assert FN in capi.EXPORTS and hasattr(lib, FN)
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'include', 'fnn.h')).read()
    assert re.search(r'^int fnn_mesh_decimate\(', header, re.M)
    assert len({r[0] for r in ROWS}) == len(ROWS)


def test_a_model_without_triangles_is_zeros_and_no_launch():
    lib = capi.load_library()
    before = _HOST.copy()
    for args in (_with(GOOD, 4, 0), _with(GOOD, 1, 0, 4, 0, 5, i64(0, 0)), _with(GOOD, 1, 0, 4, 0, 5, i64(0), 6, 0), _with(GOOD, 4, 0, 8, 1, 7, 0.0)):
        counts, status = i64(*[7] * 4), i64(*[7] * 4)
        assert lib.fnn_mesh_decimate(*_with(args, 14, counts, 15, status)) == 0
        assert list(status) == [0] * 4 and list(counts)[:2 * args[6]] == [0] * (2 * args[6])
    assert np.array_equal(_HOST, before)


# ---- the Python layer: every refusal comes before any GPU call (none of these needs a GPU)
SEG = np.zeros((3, 4, 5), np.uint8)
BAD_FACTORS = {'negative': -0.01, 'one': 1.0, 'above-one': 1.2, 'nan': math.nan, 'inf': math.inf}
MODEL = meshing.SurfaceModel(np.zeros((3, 3), np.float32), np.array([[0, 1, 2]], np.int32), np.zeros(1, np.uint16), [(1,)], np.array([0, 3]),
                             np.array([0, 1]))


@pytest.fixture
def no_gpu_call(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError('a GPU call was made before the refusal')
    for name in ('mesh_count', 'mesh_emit', 'mesh_decimate'):
        monkeypatch.setattr(capi, name, refuse)
    monkeypatch.setattr(meshing, '_device', refuse)
    monkeypatch.setattr(meshing, '_to_device', refuse)


@pytest.mark.parametrize('name', list(BAD_FACTORS))
def test_a_bad_factor_is_refused_before_any_gpu_call(name, no_gpu_call, tmp_path):
    d = BAD_FACTORS[name]
    with pytest.raises(ValueError, match=r'decimation_factor must lie in \[0, 1\)'):
        meshing.label_surfaces(SEG, decimation_factor=d)
    with pytest.raises(ValueError, match=r'decimation_factor must lie in \[0, 1\)'):
        meshing.decimate_surfaces(MODEL, d)
    gen, out = meshing.VTKModelGenerator(decimation=True), str(tmp_path / 'm.vtk')
    with pytest.raises(ValueError, match=r'decimation_factor must lie in \[0, 1\)'):
        gen.generate_vtk_model('mask.nii.gz', out, decimation_factor=d)
    with pytest.raises(ValueError, match=r'decimation_factor must lie in \[0, 1\)'):
        gen.generate_from_labels(SEG, {}, out, decimation_factor=d)
    assert not os.path.exists(out)


def test_a_model_that_does_not_fit_itself_is_refused_before_any_gpu_call(no_gpu_call):
    import dataclasses
    for change in (dict(point_offsets=np.array([0, 2])), dict(triangle_region=np.zeros(2, np.uint16)), dict(triangles=np.array([[0, 1, 3]], np.int32)),
                   dict(triangle_region=np.ones(1, np.uint16)), dict(regions=[(1,), (2,)])):
        with pytest.raises(ValueError, match='model'):
            meshing.decimate_surfaces(dataclasses.replace(MODEL, **change), 0.5)


def test_the_default_generator_still_refuses_decimation_and_says_how_to_get_it(no_gpu_call, tmp_path):
    gen, out = meshing.VTKModelGenerator(), str(tmp_path / 'm.vtk')
    assert gen.decimation is False and meshing.VTKModelGenerator(decimation=True).decimation is True
    for call_ in (lambda **k: gen.generate_vtk_model('mask.nii.gz', out, **k), lambda **k: gen.generate_from_labels(SEG, {}, out, **k)):
        with pytest.raises(NotImplementedError, match=r'decimation_factor=0\.2.*decimation=True'):
            call_(decimation_factor=0.2)
        with pytest.raises(NotImplementedError, match='decimation=True'):
            call_(decimation_factor=1.5)                             # it does not look at the value: the old behaviour
    model = meshing.SurfaceModel(*[None] * 6)
    assert model.rounds == 0 and model.exhausted == 0
