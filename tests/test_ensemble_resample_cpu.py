"""fnn_ensemble_resample_export and the ensemble's file methods, as far as they go without a GPU: the entry is declared,
exported and additive; every refusal comes before a launch with its code and its fnn_last_error(NULL) text (no machine
without a GPU owns device memory, so a call that passes them all ends at the device-pointer refusal);
``plan_ensemble_export`` on combinations of the four ``plan_label_export`` paths; what ``predict_from_files`` refuses
when it starts."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from fast_nnunet_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED = capi.FNN_E_INVALID, capi.FNN_E_UNSUPPORTED
F16, F32, U8, U16 = capi.FNN_OUT_F16, capi.FNN_OUT_F32, capi.FNN_LABEL_U8, capi.FNN_LABEL_U16
DEFAULT, TORCH = capi.FNN_RESAMPLE_DEFAULT, capi.FNN_RESAMPLE_TORCH
FN = 'fnn_ensemble_resample_export'

_HOST = np.zeros(1 << 14, np.uint8)
_BASE = (_HOST.ctypes.data + 63) & ~63          # host memory, 64-byte aligned


def hp(off=0):
    return C.c_void_p(_BASE + off)


def i64(*v):
    return (C.c_int64 * len(v))(*v)


def i32(*v):
    return (C.c_int32 * len(v))(*v)


def members(*rows):
    """rows of (pointer, shape, dtype, family, separate_axis) -> fnn_ensemble_member[]"""
    table = (capi.EnsembleMember * len(rows))()
    for e, (ptr, shape, dtype, family, sep) in zip(table, rows):
        e.logits, e.shape, e.dtype, e.family, e.separate_axis = ptr.value, i64(*shape), dtype, family, sep
    return table


NULL = None
ONE = (hp(), (4, 5, 6), F16, DEFAULT, -1)
BBOX, BEFORE, TB = i64(1, 7, 0, 8, 2, 9), i64(8, 8, 10), i32(0, 1, 2)
#       members      n  heads order bbox  before  tb  avg   labels    label dtype stream
GOOD = (members(ONE), 1, 3, NULL, BBOX, BEFORE, TB, NULL, hp(8192), U8, NULL)
DEVMSG = FN + ' needs device pointers (no CPU path)'


def _with(args, k, v):
    return args[:k] + (v,) + args[k + 1:]


def _member(**kw):
    row = dict(zip(('ptr', 'shape', 'dtype', 'family', 'sep'), ONE))
    row.update(kw)
    return _with(GOOD, 0, members(tuple(row[k] for k in ('ptr', 'shape', 'dtype', 'family', 'sep'))))


ROWS = [(f'null-{k}', _with(GOOD, k, NULL), INVALID, 'NULL argument') for k in (0, 4, 5, 6, 8)]
ROWS += [('host', GOOD, INVALID, DEVMSG),
         ('host-avg', _with(GOOD, 7, hp(4096)), INVALID, DEVMSG),
         ('host-regions-u16', _with(_with(GOOD, 3, i32(1, 2, 3)), 9, U16), INVALID, DEVMSG),
         ('members0', _with(GOOD, 1, 0), INVALID, 'n_members must be 1..16'),
         ('members-negative', _with(GOOD, 1, -1), INVALID, 'n_members must be 1..16'),
         ('members17', _with(_with(GOOD, 0, members(*[ONE] * 17)), 1, 17), INVALID, 'n_members must be 1..16'),
         ('members16-host', _with(_with(GOOD, 0, members(*[ONE] * 16)), 1, 16), INVALID, DEVMSG),
         ('heads0', _with(GOOD, 2, 0), INVALID, 'heads must be at least 1'),
         ('heads-negative', _with(GOOD, 2, -4), INVALID, 'heads must be at least 1'),
         ('label-dtype', _with(GOOD, 9, 2), INVALID, 'unknown label dtype'),
         ('member-null-logits', _member(ptr=C.c_void_p(0)), INVALID, 'NULL member logits'),
         ('member-dtype', _member(dtype=2), INVALID, 'unknown member logits dtype'),
         ('member-shape0', _member(shape=(4, 0, 6)), INVALID, 'bad shape'),
         ('member-shape-negative', _member(shape=(-1, 5, 6)), INVALID, 'bad shape'),
         ('member-family', _member(family=2), UNSUPPORTED, 'unknown resampling family'),
         ('member-family-negative', _member(family=-1), UNSUPPORTED, 'unknown resampling family'),
         ('member-sep3', _member(sep=3), INVALID, 'separate_axis must be -1 .. 2'),
         ('member-sep-2', _member(sep=-2), INVALID, 'separate_axis must be -1 .. 2'),
         ('second-member-family', _with(_with(GOOD, 0, members(ONE, (hp(), (4, 5, 6), F32, 7, -1))), 1, 2), UNSUPPORTED,
          'unknown resampling family'),
         ('member-axis-too-long', _member(shape=((1 << 24) + 1, 5, 6)), UNSUPPORTED,
          'an axis longer than 2^24 is not implemented (float32 coordinates)'),
         ('extent-too-long', _with(_with(GOOD, 4, i64(0, (1 << 24) + 1, 0, 8, 2, 9)), 5, i64(1 << 25, 8, 10)), UNSUPPORTED,
          'an axis longer than 2^24 is not implemented (float32 coordinates)'),
         ('plane-too-large', _with(_with(GOOD, 4, i64(0, 2, 0, 1 << 16, 0, 1 << 16)), 5, i64(2, 1 << 16, 1 << 16)), UNSUPPORTED,
          'output too large for one launch'),
         ('permutation', _with(GOOD, 6, i32(0, 0, 1)), INVALID, 'transpose_backward is not a permutation of (0, 1, 2)'),
         ('permutation-3', _with(GOOD, 6, i32(1, 2, 3)), INVALID, 'transpose_backward is not a permutation of (0, 1, 2)'),
         ('bbox-outside', _with(GOOD, 4, i64(1, 9, 0, 8, 2, 9)), INVALID, 'bbox outside shape_before_cropping'),
         ('bbox-negative', _with(GOOD, 4, i64(-1, 7, 0, 8, 2, 9)), INVALID, 'bbox outside shape_before_cropping'),
         ('bbox-empty', _with(GOOD, 4, i64(3, 3, 0, 8, 2, 9)), INVALID, 'bbox outside shape_before_cropping'),
         ('heads257-u8', _with(GOOD, 2, 257), INVALID, 'more than 256 heads need uint16 labels'),
         ('heads256-u8-host', _with(GOOD, 2, 256), INVALID, DEVMSG),
         ('heads300-u8-regions-host', _with(_with(GOOD, 2, 300), 3, i32(*range(300))), INVALID, DEVMSG),
         ('heads640-u16-host', _with(_with(GOOD, 2, 640), 9, U16), INVALID, DEVMSG),
         ('heads641-u16', _with(_with(GOOD, 2, 641), 9, U16), UNSUPPORTED,
          "more than 640 heads: a voxel's running sums do not fit the LDS of a CU"),
         ('heads4097-regions', _with(_with(GOOD, 2, 4097), 3, i32(*range(4097))), UNSUPPORTED,
          "more than 640 heads: a voxel's running sums do not fit the LDS of a CU")]


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
    assert re.search(r'\bint\s+' + FN + r'\s*\(', header) and 'typedef struct fnn_ensemble_member {' in header
    assert C.sizeof(capi.EnsembleMember) == 48                  # pointer, int64[3], 3 x int32, padded to 8
    assert len({r[0] for r in ROWS}) == len(ROWS)


def test_the_python_call_raises_with_the_message():
    """capi.check maps the codes onto the exception types the reference raises: FNN_E_UNSUPPORTED is NotImplementedError,
    FNN_E_INVALID AssertionError."""
    with pytest.raises(NotImplementedError, match='unknown resampling family'):
        capi.ensemble_resample_export([(_BASE, True, (4, 5, 6), 5, None)], 3, None, [[1, 7], [0, 8], [2, 9]], (8, 8, 10),
                                      (0, 1, 2), None, _BASE + 8192, False)
    with pytest.raises(AssertionError, match='no CPU path'):
        capi.ensemble_resample_export([(_BASE, True, (4, 5, 6), DEFAULT, 0), (_BASE, False, (6, 8, 7), TORCH, None)], 3,
                                      [1, 2, 3], [[1, 7], [0, 8], [2, 9]], (8, 8, 10), (2, 0, 1), _BASE + 4096, _BASE + 8192, True)


# ---- plan_ensemble_export ----------------------------------------------------------------------------------------------
def _plans():
    """The four paths of plan_label_export, made by plan_label_export."""
    from fast_nnunet_amd.preprocess import DEFAULT_RESAMPLING_FN, NO_RESAMPLING_FNS, TORCH_RESAMPLING_FN, plan_label_export
    iso, low = [1.0, 1.0, 1.0], [2.0, 2.0, 2.0]
    kw1 = {'is_seg': False, 'order': 1, 'order_z': 0, 'force_separate_z': None}
    plans = {'same-grid': plan_label_export(DEFAULT_RESAMPLING_FN, kw1, iso, iso, (8, 8, 8), (8, 8, 8)),
             'same-grid-none': plan_label_export(NO_RESAMPLING_FNS[0], {}, low, iso, (4, 4, 4), (8, 8, 8)),
             'fused-default': plan_label_export(DEFAULT_RESAMPLING_FN, kw1, low, iso, (4, 4, 4), (8, 8, 8)),
             'fused-default-sep': plan_label_export(DEFAULT_RESAMPLING_FN, kw1, [5.0, 1.0, 1.0], [5.0, 0.5, 0.5], (4, 4, 4), (4, 8, 8)),
             'fused-torch': plan_label_export(TORCH_RESAMPLING_FN, {'is_seg': False}, low, iso, (4, 4, 4), (8, 8, 8)),
             'two-step': plan_label_export(DEFAULT_RESAMPLING_FN, dict(kw1, order=3), low, iso, (4, 4, 4), (8, 8, 8)),
             'two-step-order_z': plan_label_export(DEFAULT_RESAMPLING_FN, dict(kw1, order_z=1), low, iso, (4, 4, 4), (8, 8, 8))}
    assert {k: v['path'] for k, v in plans.items()} == {
        'same-grid': 'same-grid', 'same-grid-none': 'same-grid', 'fused-default': 'fused-default',
        'fused-default-sep': 'fused-default', 'fused-torch': 'fused-torch', 'two-step': 'two-step',
        'two-step-order_z': 'two-step'}
    assert plans['fused-default-sep']['separate_axis'] == 0
    return plans


def test_plan_ensemble_export_on_combinations_of_the_paths():
    import itertools
    from fast_nnunet_amd.preprocess import plan_ensemble_export
    plans = _plans()
    for n in (1, 2, 3):
        for combo in itertools.product(plans, repeat=n):
            want = 'two-step' if any(c.startswith('two-step') for c in combo) else 'fused'
            assert plan_ensemble_export([plans[c] for c in combo]) == want, combo
    assert plan_ensemble_export(plans[c] for c in ('same-grid', 'fused-torch')) == 'fused'       # any iterable
    assert plan_ensemble_export([plans['fused-default']] * 16) == 'fused'
    with pytest.raises(ValueError):
        plan_ensemble_export([])
    with pytest.raises(ValueError):
        plan_ensemble_export([{'path': 'fused', 'separate_axis': None}])


def test_a_refusal_of_plan_resampling_stays_a_refusal():
    from fast_nnunet_amd.preprocess import TORCH_RESAMPLING_FN, plan_ensemble_export, plan_label_export
    iso, low = [1.0, 1.0, 1.0], [2.0, 2.0, 2.0]
    with pytest.raises(NotImplementedError):
        plan_ensemble_export([plan_label_export(TORCH_RESAMPLING_FN, {'mode': 'bicubic'}, low, iso, (4, 4, 4), (8, 8, 8))])
    with pytest.raises(RuntimeError):
        plan_ensemble_export([plan_label_export('resample_magic', {}, low, iso, (4, 4, 4), (8, 8, 8))])


# ---- what the file methods refuse before any GPU work ------------------------------------------------------------------
def _cpu_member(file_ending='.nii.gz', previous_stage=None, reader_writer=None):
    """A member as far as the ensemble looks at it before the first case: plans, labels and dataset.json, no engine
    (constructing a predictor touches no GPU)."""
    from fast_nnunet_amd import nnUNetPredictor
    from fast_nnunet_amd.plans import PlansManager
    conf = {'patch_size': [16, 16, 16], 'spacing': [1.0, 1.0, 1.0], 'normalization_schemes': ['CTNormalization'],
            'use_mask_for_norm': [False],
            'architecture': {'network_class_name': 'PlainConvUNet', 'arch_kwargs': {}, '_kw_requires_import': []}}
    confs = {'3d_fullres': conf, '3d_lowres': dict(conf, spacing=[2.0, 2.0, 2.0]),
             '3d_cascade_fullres': dict(conf, previous_stage='3d_lowres')}
    pm = PlansManager({'dataset_name': 'Dataset995_EnsembleFiles', 'plans_name': 'nnUNetPlans', 'transpose_forward': [0, 1, 2],
                       'transpose_backward': [0, 1, 2], 'configurations': confs})
    dj = {'labels': {'background': 0, 'a': 1, 'b': 2}, 'channel_names': {'0': 'CT'}, 'file_ending': file_ending}
    if reader_writer is not None:
        dj['overwrite_image_reader_writer'] = reader_writer
    p = nnUNetPredictor(device='cuda', allow_tqdm=False)
    p.plans_manager, p.dataset_json, p.label_manager = pm, dj, pm.get_label_manager(dj)
    p.configuration_manager = pm.get_configuration('3d_cascade_fullres' if previous_stage else '3d_fullres')
    return p


def test_the_ensemble_has_the_predictors_file_methods():
    import inspect
    from fast_nnunet_amd import nnUNetPredictor
    from fast_nnunet_amd.ensembling import nnUNetEnsemblePredictor
    for name in ('predict_from_files', 'predict_from_files_sequential'):
        assert inspect.signature(getattr(nnUNetEnsemblePredictor, name)) == inspect.signature(getattr(nnUNetPredictor, name))
    ens = nnUNetEnsemblePredictor([_cpu_member(), _cpu_member()])
    assert ens.export_stats == {'fused': 0, 'two-step': 0} and ens.compress_on_device is False
    assert isinstance(ens.fused_export, bool)
    assert nnUNetEnsemblePredictor([_cpu_member()], fused_export=False, compress_on_device=True).compress_on_device is True


def test_members_of_different_file_types_are_refused_when_the_call_starts(tmp_path):
    from fast_nnunet_amd.ensembling import nnUNetEnsemblePredictor
    ens = nnUNetEnsemblePredictor([_cpu_member('.nii.gz'), _cpu_member('.nii')])        # (not in the constructor)
    for method in (ens.predict_from_files, ens.predict_from_files_sequential):
        with pytest.raises(ValueError, match='file endings'):
            method([[str(tmp_path / 'case_0000.nii.gz')]], str(tmp_path / 'out'))
    ens = nnUNetEnsemblePredictor([_cpu_member(), _cpu_member(reader_writer='NibabelIOWithReorient')])
    for method in (ens.predict_from_files, ens.predict_from_files_sequential):
        with pytest.raises(ValueError, match='read and write images differently'):
            method([[str(tmp_path / 'case_0000.nii.gz')]], str(tmp_path / 'out'))
    assert not (tmp_path / 'out').exists(), 'refused before the output folder was made'


def test_previous_stage_folders_are_one_per_member(tmp_path):
    from fast_nnunet_amd.ensembling import nnUNetEnsemblePredictor
    ens = nnUNetEnsemblePredictor([_cpu_member(), _cpu_member(previous_stage=True)])
    case = [[str(tmp_path / 'case_0000.nii.gz')]]
    for folders in ([str(tmp_path)], [None, str(tmp_path), None], str(tmp_path)):
        with pytest.raises(ValueError, match='one entry per member'):
            ens.predict_from_files(case, str(tmp_path / 'out'), folder_with_segs_from_prev_stage=folders)
        with pytest.raises(ValueError, match='one entry per member'):
            ens.predict_from_files_sequential(case, str(tmp_path / 'out'), folder_with_segs_from_prev_stage=folders)
    # a cascade member without its folder fails the reference's assertion
    for folders in (None, [str(tmp_path), None]):
        with pytest.raises(AssertionError, match='cascaded network'):
            ens.predict_from_files(case, None, folder_with_segs_from_prev_stage=folders)
    # the lists: the previous stage's file of every member, per case
    cases, truncated, prev = ens._manage_input_and_output_lists(
        [[str(tmp_path / 'a_0000.nii.gz')], [str(tmp_path / 'b_0000.nii.gz')], [str(tmp_path / 'c_0000.nii.gz')]],
        str(tmp_path / 'out'), [None, str(tmp_path / 'low')], True, 1, 2, False)
    assert [os.path.basename(t) for t in truncated] == ['b'] and prev == [[None, str(tmp_path / 'low' / 'b.nii.gz')]]
    assert ens._manage_input_and_output_lists(cases, None, None)[1:] == (None, [None])
