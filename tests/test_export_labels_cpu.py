"""The label export's decision without a GPU: which path ``plan_label_export`` picks for a configuration's
``resampling_fn_probabilities`` (the fused pass of ``fnn_resample_labels`` only where it computes what the two-step route
computes: order 1 / order_z 0 of the default family, the torch family), and the C ABI's symbol list."""
import pytest

from fast_nnunet_amd import capi
from fast_nnunet_amd.preprocess import (DEFAULT_RESAMPLING_FN, NO_RESAMPLING_FNS, TORCH_RESAMPLING_FN, plan_label_export)

ISO = [1.0, 1.0, 1.0]
IN, OUT = (9, 7, 11), (13, 10, 17)
DEFAULT_KW = {'is_seg': False, 'order': 1, 'order_z': 0, 'force_separate_z': None}
TORCH_KW = {'is_seg': False, 'force_separate_z': None, 'memefficient_seg_resampling': False,
            'separate_z_anisotropy_threshold': 3}


def _aniso(axis):
    sp = [1.0, 1.0, 1.0]
    sp[axis] = 5.0
    return sp


def test_the_library_exports_the_entry():
    assert 'fnn_resample_labels' in capi.EXPORTS
    assert (capi.FNN_RESAMPLE_DEFAULT, capi.FNN_RESAMPLE_TORCH) == (0, 1)


@pytest.mark.parametrize('order,path', [(0, 'two-step'), (1, 'fused-default'), (3, 'two-step')])
def test_default_family_orders(order, path):
    got = plan_label_export(DEFAULT_RESAMPLING_FN, dict(DEFAULT_KW, order=order), ISO, ISO, IN, OUT)
    assert got == {'path': path, 'separate_axis': None}


def test_default_family_without_kwargs_is_the_cubic():
    # resample() reads a missing order as 3
    assert plan_label_export(DEFAULT_RESAMPLING_FN, None, ISO, ISO, IN, OUT)['path'] == 'two-step'


def test_default_family_order_z_1_stays_two_step():
    got = plan_label_export(DEFAULT_RESAMPLING_FN, dict(DEFAULT_KW, order_z=1), _aniso(0), ISO, IN, OUT)
    assert got == {'path': 'two-step', 'separate_axis': 0}


@pytest.mark.parametrize('fn,kw,path', [(DEFAULT_RESAMPLING_FN, DEFAULT_KW, 'fused-default'),
                                        (TORCH_RESAMPLING_FN, TORCH_KW, 'fused-torch')])
@pytest.mark.parametrize('axis', [0, 1, 2])
def test_each_separate_axis(fn, kw, path, axis):
    # anisotropic current spacing, and anisotropic new spacing alone
    assert plan_label_export(fn, kw, _aniso(axis), ISO, IN, OUT) == {'path': path, 'separate_axis': axis}
    assert plan_label_export(fn, kw, ISO, _aniso(axis), IN, OUT) == {'path': path, 'separate_axis': axis}
    # force_separate_z=False switches it off; two equally coarse axes are no separate axis
    assert plan_label_export(fn, dict(kw, force_separate_z=False), _aniso(axis), ISO, IN, OUT)['separate_axis'] is None
    two = _aniso(axis)
    two[(axis + 1) % 3] = 5.0
    assert plan_label_export(fn, kw, two, ISO, IN, OUT) == {'path': path, 'separate_axis': None}


def test_torch_family():
    assert plan_label_export(TORCH_RESAMPLING_FN, TORCH_KW, ISO, ISO, IN, OUT) == {'path': 'fused-torch', 'separate_axis': None}
    assert plan_label_export(TORCH_RESAMPLING_FN, None, ISO, ISO, IN, OUT)['path'] == 'fused-torch'
    with pytest.raises(NotImplementedError):
        plan_label_export(TORCH_RESAMPLING_FN, dict(TORCH_KW, mode='cubic'), ISO, ISO, IN, OUT)
    with pytest.raises(NotImplementedError):
        plan_label_export(TORCH_RESAMPLING_FN, dict(TORCH_KW, aniso_axis_mode='linear'), _aniso(0), ISO, IN, OUT)
    with pytest.raises(TypeError):
        plan_label_export(TORCH_RESAMPLING_FN, dict(TORCH_KW, order=1), ISO, ISO, IN, OUT)


@pytest.mark.parametrize('fn,kw', [(DEFAULT_RESAMPLING_FN, DEFAULT_KW), (TORCH_RESAMPLING_FN, TORCH_KW),
                                   (DEFAULT_RESAMPLING_FN, dict(DEFAULT_KW, order=3))])
def test_equal_grids_resample_nothing(fn, kw):
    assert plan_label_export(fn, kw, _aniso(0), ISO, IN, list(IN)) == {'path': 'same-grid', 'separate_axis': None}


@pytest.mark.parametrize('fn', NO_RESAMPLING_FNS)
def test_the_no_resampling_names(fn):
    assert plan_label_export(fn, {}, ISO, ISO, IN, OUT) == {'path': 'same-grid', 'separate_axis': None}


def test_an_unknown_name_raises():
    with pytest.raises(RuntimeError, match='Unable to find resampling function'):
        plan_label_export('resample_with_magic', DEFAULT_KW, ISO, ISO, IN, OUT)
