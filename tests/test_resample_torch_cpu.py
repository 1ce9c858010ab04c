"""The torch resampling family without a GPU: the restatement on top of ``torch.nn.functional.interpolate``
(tests/resample_torch_ref.py, the yardstick of the GPU tests) against vectors made by the reference's own
``resample_torch_fornnunet`` / ``resample_torch_simple`` (tests/golden/resample_torch.npz), what the plans readers
return for a torch-resampling ``plans.json``, the decision function, and the C ABI's symbol list.

Gates against the golden file (CPU results may differ in the last bit between machines, so no float equality):
images within 4 * 6e-8 * max|x| - a few float32 steps of the data range, the project's resampling tolerance; label
maps equal except at near-ties of the helper's own scores (two best fp16 scores within 0.5, |score - 0.5| <= 2^-20
for the memefficient rule), where the golden label must be one of the two best; near-ties at most 2 % of a case."""
import os

import numpy as np
import pytest
import torch

import resample_torch_ref as rt

TORCH_KW = {'is_seg': False, 'force_separate_z': None, 'memefficient_seg_resampling': False,
            'separate_z_anisotropy_threshold': 3}


@pytest.fixture(scope='module')
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, 'resample_torch.npz'))


@pytest.mark.parametrize('axis', [None, 0, 1, 2])
def test_helper_matches_the_reference_on_images(golden, axis):
    x, new_shape = golden['image__in'], golden['new_shape']
    want = golden['image__out' if axis is None else f'image__sep{axis}']
    got = rt.resample(x, new_shape, axis).numpy()
    assert got.dtype == np.float32 and got.shape == want.shape
    err = np.abs(got - want).max()
    print(f'axis {axis}: max|err| {err:.3g}')
    assert err <= 4 * 6e-8 * np.abs(x).max()


@pytest.mark.parametrize('axis', [None, 0, 1, 2])
@pytest.mark.parametrize('memefficient', [False, True], ids=['argmax', 'memeff'])
@pytest.mark.parametrize('labels', ['few', 'sparse'])
def test_helper_matches_the_reference_on_segmentations(golden, labels, memefficient, axis):
    seg, new_shape = golden[f'seg_{labels}__in'], golden['new_shape']
    tag = ('memeff' if memefficient else 'argmax') + ('' if axis is None else f'_sep{axis}')
    want = golden[f'seg_{labels}__{tag}']
    values, scores = rt.seg_scores(seg, new_shape, axis, memefficient)
    share, diff = rt.check_labels(want, values, scores, memefficient)
    print(f'{labels} {tag}: near-tie share {share:.4f}, labels off the yardstick {diff}')
    got = rt.resample(seg, new_shape, axis, is_seg=True, memefficient=memefficient).numpy()
    assert got.dtype == np.int16
    rt.check_labels(got, values, scores, memefficient)


def test_the_references_separate_branch_raises(golden):
    """Why the separate-z vectors come from resample_torch_simple: recorded when the golden file was made."""
    assert int(golden['separate_branch_raises']) == 1


def _cm(extra):
    from fast_nnunet_amd.plans import PlansManager
    cfg = {'patch_size': [16, 16, 16], 'spacing': [1.0, 1.0, 1.0],
           'architecture': {'network_class_name': 'PlainConvUNet', 'arch_kwargs': {}, '_kw_requires_import': []}}
    cfg.update(extra)
    pm = PlansManager({'dataset_name': 'Dataset998_TorchRes', 'plans_name': 'nnUNetPlans_torchres',
                       'configurations': {'3d_fullres': cfg}})
    return pm.get_configuration('3d_fullres')


def test_plans_expose_the_torch_resampling_of_a_configuration():
    seg_kw = dict(TORCH_KW, is_seg=True)
    cm = _cm({'resampling_fn_data': 'resample_torch_fornnunet', 'resampling_fn_data_kwargs': TORCH_KW,
              'resampling_fn_seg': 'resample_torch_fornnunet', 'resampling_fn_seg_kwargs': seg_kw,
              'resampling_fn_probabilities': 'resample_torch_fornnunet', 'resampling_fn_probabilities_kwargs': TORCH_KW})
    assert cm.resampling_fn_data_name == cm.resampling_fn_seg_name == cm.resampling_fn_probabilities_name \
        == 'resample_torch_fornnunet'
    assert cm.resampling_fn_seg_kwargs == seg_kw and cm.resampling_fn_data_kwargs == TORCH_KW
    default = _cm({})
    assert default.resampling_fn_seg_name == 'resample_data_or_seg_to_shape'
    assert default.resampling_fn_seg_kwargs == {'is_seg': True, 'order': 1, 'order_z': 0, 'force_separate_z': None}
    assert default.resampling_fn_data_kwargs == {'is_seg': False, 'order': 3, 'order_z': 0, 'force_separate_z': None}


def test_dispatch_maps_the_function_names():
    from fast_nnunet_amd.preprocess import plan_resampling
    iso, aniso = (1.0, 1.0, 1.0), (5.0, 1.0, 1.0)
    assert plan_resampling('resample_data_or_seg_to_shape', {'is_seg': False, 'order': 3}, iso, iso) == {'path': 'default'}
    assert plan_resampling('no_resampling_data_or_seg_to_shape', {}, iso, iso) == {'path': 'none'}
    assert plan_resampling('resample_torch_fornnunet', TORCH_KW, iso, iso) == \
        {'path': 'torch', 'separate_axis': None, 'memefficient': False}
    # anisotropic current spacing: the low-resolution axis; forced off; forced on; a higher threshold
    assert plan_resampling('resample_torch_fornnunet', TORCH_KW, aniso, iso)['separate_axis'] == 0
    assert plan_resampling('resample_torch_fornnunet', TORCH_KW, (1.0, 1.0, 4.0), iso)['separate_axis'] == 2
    assert plan_resampling('resample_torch_fornnunet', TORCH_KW, iso, (1.0, 3.5, 1.0))['separate_axis'] == 1
    assert plan_resampling('resample_torch_fornnunet', dict(TORCH_KW, force_separate_z=False), aniso, iso)['separate_axis'] is None
    assert plan_resampling('resample_torch_fornnunet', dict(TORCH_KW, force_separate_z=True), (1.0, 1.2, 1.0), iso)['separate_axis'] == 1
    assert plan_resampling('resample_torch_fornnunet', dict(TORCH_KW, separate_z_anisotropy_threshold=6), aniso, iso)['separate_axis'] is None
    assert plan_resampling('resample_torch_fornnunet', dict(TORCH_KW, is_seg=True, memefficient_seg_resampling=True),
                           iso, iso)['memefficient'] is True
    # accepted and ignored
    kw = dict(TORCH_KW, num_threads=8, device='cpu', mode='linear', aniso_axis_mode='nearest-exact')
    assert plan_resampling('resample_torch_fornnunet', kw, iso, iso)['path'] == 'torch'


def test_dispatch_refuses_what_is_not_implemented():
    from fast_nnunet_amd.preprocess import plan_resampling
    iso = (1.0, 1.0, 1.0)
    with pytest.raises(RuntimeError, match='resample_with_scipy_magic'):
        plan_resampling('resample_with_scipy_magic', {}, iso, iso)
    with pytest.raises(NotImplementedError, match='mode'):
        plan_resampling('resample_torch_fornnunet', dict(TORCH_KW, mode='bicubic'), iso, iso)
    with pytest.raises(NotImplementedError, match='aniso_axis_mode'):
        plan_resampling('resample_torch_fornnunet', dict(TORCH_KW, aniso_axis_mode='nearest'), iso, iso)
    with pytest.raises(TypeError, match='order'):
        plan_resampling('resample_torch_fornnunet', dict(TORCH_KW, order=3), iso, iso)


def test_the_new_entry_points_are_exported():
    from fast_nnunet_amd import capi
    assert {'fnn_resample_torch', 'fnn_resample_torch_seg'} <= set(capi.EXPORTS)
    lib = capi.load_library()
    assert hasattr(lib, 'fnn_resample_torch') and hasattr(lib, 'fnn_resample_torch_seg')
    assert lib.fnn_abi_version() == 4
    # host pointers and bad descriptors are refused before anything is launched (no GPU needed)
    import ctypes as C
    buf = np.zeros(8, np.float32)
    d = capi.ResampleTorchDesc(capi.FNN_OUT_F32, -1, 0, capi.FNN_INTERP_OTHER, capi.FNN_INTERP_NEAREST_EXACT)
    shape, new = (C.c_int64 * 4)(1, 2, 2, 2), (C.c_int64 * 3)(2, 2, 2)
    assert lib.fnn_resample_torch(buf.ctypes.data, shape, new, C.byref(d), buf.ctypes.data, None) == capi.FNN_E_UNSUPPORTED
    d.mode, d.aniso_axis_mode = capi.FNN_INTERP_LINEAR, capi.FNN_INTERP_LINEAR
    assert lib.fnn_resample_torch_seg(buf.ctypes.data, shape, new, C.byref(d), buf.ctypes.data, None) == capi.FNN_E_UNSUPPORTED
    d.aniso_axis_mode = capi.FNN_INTERP_NEAREST_EXACT
    assert lib.fnn_resample_torch(None, shape, new, C.byref(d), buf.ctypes.data, None) == capi.FNN_E_INVALID
    d.separate_axis = 3
    assert lib.fnn_resample_torch(buf.ctypes.data, shape, new, C.byref(d), buf.ctypes.data, None) == capi.FNN_E_INVALID
