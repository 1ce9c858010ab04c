"""Cross-configuration ensembling without a GPU: the numpy restatement against vectors made by the reference's own
average_probabilities + convert_logits_to_segmentation (tests/golden/make_golden_ensemble.py), the .npz loader, and the
argument checks of fnn_ensemble_export / fnn_average_probabilities that come before any device work."""
import ctypes as C
import os

import numpy as np
import pytest

import ensemble_ref
from golden_cases import DATASET_JSONS

CASES = {'labels_2_transposed': ('two_mod', 2), 'labels_4_crop': ('labels3', 4), 'regions_3_crop': ('regions', 3)}


@pytest.mark.parametrize('name', sorted(CASES))
def test_restatement_matches_reference_golden(golden_dir, name):
    z = np.load(os.path.join(golden_dir, 'ensemble.npz'))
    dataset, n = CASES[name]
    members = [z[f'{name}__member{m}'] for m in range(n)]
    avg = ensemble_ref.average(members)
    assert avg.dtype == np.float32 and np.array_equal(avg.view(np.uint32), z[name + '__avg'].view(np.uint32))
    seg = ensemble_ref.merge_rule(avg, DATASET_JSONS[dataset].get('regions_class_order'))
    assert np.array_equal(seg, z[name + '__seg'])


def test_golden_covers_crop_box_and_ties(golden_dir):
    z = np.load(os.path.join(golden_dir, 'ensemble.npz'))
    avg = z['labels_4_crop__avg']
    assert (avg[0] == 1).any() and (avg[1:] == 0).any()               # voxels outside the crop box
    assert (z['regions_3_crop__seg'] == 0).any() and (z['regions_3_crop__seg'] == 3).any()


def test_npz_loader_refuses_object_arrays(tmp_path):
    from fast_nnunet_amd import ensembling
    f = str(tmp_path / 'obj.npz')
    np.savez(f, probabilities=np.array([{'a': 1}, None], dtype=object))
    with pytest.raises(ValueError):
        ensembling._load_member(f)
    with pytest.raises(ValueError):
        ensembling._load_member(np.zeros((2, 3), np.float64))
    g = str(tmp_path / 'ok.npz')
    np.savez(g, probabilities=np.ones((2, 3, 4), np.float32))
    assert ensembling._load_member(g).shape == (2, 3, 4)


def test_ensemble_predictor_refuses_bad_member_lists():
    from fast_nnunet_amd.ensembling import nnUNetEnsemblePredictor
    with pytest.raises(ValueError):
        nnUNetEnsemblePredictor([])
    with pytest.raises(ValueError):
        nnUNetEnsemblePredictor([object()])


def _export_args(capi, n=2, dtypes=None, heads=3, bbox=(0, 4, 0, 4, 0, 4), shape=(4, 4, 4), tb=(0, 1, 2)):
    bufs = [C.create_string_buffer(256) for _ in range(16)]
    ptrs = (C.c_void_p * 16)(*[C.addressof(b) for b in bufs])
    dts = (C.c_int32 * 16)(*(dtypes or [capi.FNN_OUT_F16] * 16))
    return dict(ptrs=ptrs, dts=dts, n=n, heads=heads, bbox=(C.c_int64 * 6)(*bbox), shape=(C.c_int64 * 3)(*shape),
                tb=(C.c_int32 * 3)(*tb), bufs=bufs)


def test_library_refuses_bad_ensemble_arguments_without_a_gpu():
    from fast_nnunet_amd import capi
    lib = capi.load_library()
    lab = C.create_string_buffer(64)

    def call(**kw):
        a = _export_args(capi, **{k: v for k, v in kw.items() if k not in ('ptrs', 'label_dtype')})
        ptrs = kw.get('ptrs', a['ptrs'])
        return lib.fnn_ensemble_export(ptrs, a['dts'], a['n'], a['heads'], None, a['bbox'], a['shape'], a['tb'], None,
                                       lab, kw.get('label_dtype', capi.FNN_LABEL_U8), None)

    assert call(n=0) == capi.FNN_E_INVALID
    assert call(n=17) == capi.FNN_E_INVALID
    assert call(ptrs=None) == capi.FNN_E_INVALID
    assert call(ptrs=(C.c_void_p * 16)(*([None] * 16))) == capi.FNN_E_INVALID         # a NULL member
    assert call(dtypes=[7] * 16) == capi.FNN_E_INVALID
    assert call(heads=0) == capi.FNN_E_INVALID
    assert call(label_dtype=5) == capi.FNN_E_INVALID
    assert call(tb=(0, 0, 2)) == capi.FNN_E_INVALID
    assert call(tb=(0, 1, 3)) == capi.FNN_E_INVALID
    assert call(bbox=(0, 5, 0, 4, 0, 4)) == capi.FNN_E_INVALID                            # box beyond the shape
    assert call(bbox=(-1, 3, 0, 4, 0, 4)) == capi.FNN_E_INVALID
    assert call(bbox=(2, 2, 0, 4, 0, 4)) == capi.FNN_E_INVALID                            # empty box
    assert 'bbox' in capi._err(lib, None)
    # every argument right, but host buffers: there is no CPU path
    assert call() == capi.FNN_E_INVALID and 'device' in capi._err(lib, None)
    a = _export_args(capi)
    assert lib.fnn_ensemble_export(a['ptrs'], a['dts'], 2, 3, None, a['bbox'], a['shape'], a['tb'], None, None,
                                   capi.FNN_LABEL_U8, None) == capi.FNN_E_INVALID           # NULL labels
    assert lib.fnn_ensemble_export(a['ptrs'], None, 2, 3, None, a['bbox'], a['shape'], a['tb'], None, lab,
                                   capi.FNN_LABEL_U8, None) == capi.FNN_E_INVALID           # NULL dtypes


def test_library_refuses_bad_average_arguments_without_a_gpu():
    from fast_nnunet_amd import capi
    lib = capi.load_library()
    lab = C.create_string_buffer(64)
    a = _export_args(capi)
    p = a['ptrs']
    f = lib.fnn_average_probabilities
    assert f(p, 0, 3, None, 8, None, lab, capi.FNN_LABEL_U8, None) == capi.FNN_E_INVALID
    assert f(p, 17, 3, None, 8, None, lab, capi.FNN_LABEL_U8, None) == capi.FNN_E_INVALID
    assert f(None, 2, 3, None, 8, None, lab, capi.FNN_LABEL_U8, None) == capi.FNN_E_INVALID
    assert f((C.c_void_p * 2)(None, None), 2, 3, None, 8, None, lab, capi.FNN_LABEL_U8, None) == capi.FNN_E_INVALID
    assert f(p, 2, 0, None, 8, None, lab, capi.FNN_LABEL_U8, None) == capi.FNN_E_INVALID
    assert f(p, 2, 3, None, -1, None, lab, capi.FNN_LABEL_U8, None) == capi.FNN_E_INVALID
    assert f(p, 2, 3, None, 8, None, lab, 9, None) == capi.FNN_E_INVALID
    assert f(p, 2, 3, None, 8, None, None, capi.FNN_LABEL_U8, None) == capi.FNN_E_INVALID
    assert f(p, 2, 3, None, 8, None, lab, capi.FNN_LABEL_U8, None) == capi.FNN_E_INVALID   # host buffers
    assert 'device' in capi._err(lib, None)
