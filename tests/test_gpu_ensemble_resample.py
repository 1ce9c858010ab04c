"""fnn_ensemble_resample_export (csrc/ensemble_resample.hip) on a real MI355X: the ensemble's average and labels straight
from the members' network grids must be bit for bit what the merged route writes - every member resampled to the box's
extents by fnn_resample (order 1, order_z 0) or fnn_resample_torch, or taken as it is when the grids agree, then
fnn_ensemble_export.  That route runs on the device next to the entry under test in every case.  Then
nnUNetEnsemblePredictor with the fused step against the two-step one and against the members' own exports, and its file
methods against the array route, a single member's files and ensemble_folders."""
import gzip
import os
import pickle
import re

import numpy as np
import pytest
import torch

import ensemble_ref
from test_gpu_ensembling import _ensemble, _labels_np, _member, _member_logits, _stream

pytestmark = pytest.mark.gpu

F16, F32 = True, False
D, T = 0, 1                                        # capi.FNN_RESAMPLE_DEFAULT / FNN_RESAMPLE_TORCH
SEEN = set()                                       # what fnn_op_last_kernels named after the calls of this file


def _resampled(lg, family, sep, extents):
    """Today's step for one member: its logits on the box's extents, in its own dtype."""
    from fast_nnunet_amd import capi
    if list(lg.shape[1:]) == list(extents):
        return lg
    out = torch.empty((lg.shape[0], *extents), dtype=lg.dtype, device='cuda')
    if family == D:
        capi.resample(lg.data_ptr(), lg.shape, extents, 1, sep, lg.dtype == torch.half, out.data_ptr(), _stream(), order_z=0)
    else:
        capi.resample_torch(lg.data_ptr(), lg.shape, extents, sep, lg.dtype == torch.half, out.data_ptr(), _stream())
    return out


def _fused(lgs, specs, heads, order, bbox, before, tb, u16=False, with_avg=True):
    from fast_nnunet_amd import capi
    grid = [before[j] for j in tb]
    avg = torch.empty((heads, *grid), dtype=torch.float32, device='cuda') if with_avg else None
    labels = torch.empty(grid, dtype=torch.int16 if u16 else torch.uint8, device='cuda')
    capi.ensemble_resample_export([(lg.data_ptr(), lg.dtype == torch.half, lg.shape[1:], fam, sep)
                                   for lg, (_, _, fam, sep) in zip(lgs, specs)], heads, order, bbox, before, tb,
                                  None if avg is None else avg.data_ptr(), labels.data_ptr(), u16, _stream())
    assert capi.op_last_kernels() == ['ensemble_resample_kernel']
    SEEN.update(capi.op_last_kernels())
    return avg, labels


def _check(name, specs, heads, order, before, bbox, tb, lgs=None):
    """specs: one (network grid, half, family, separate axis) per member -> (the members' logits, average, labels)."""
    u16 = heads > 255
    extents = [hi - lo for lo, hi in bbox]
    if lgs is None:
        lgs = [_member_logits(100 * len(name) + m, heads, s[0], s[1]) for m, s in enumerate(specs)]
    want_avg, want_labels = _ensemble([_resampled(lg, s[2], s[3], extents) for lg, s in zip(lgs, specs)], heads, order,
                                      bbox, before, tb, u16)
    avg, labels = _fused(lgs, specs, heads, order, bbox, before, tb, u16)
    assert torch.equal(avg.view(torch.int32), want_avg.view(torch.int32)), name
    assert torch.equal(labels, want_labels), name
    _, labels_only = _fused(lgs, specs, heads, order, bbox, before, tb, u16, with_avg=False)
    assert torch.equal(labels_only, labels), name
    if order is None:                                           # the crafted ties are decided by the first maximum
        assert (_labels_np(labels, u16) == 0).any(), name
    return lgs, avg, labels


E = (8, 10, 14)                                    # the extents of most cases, inside BEFORE on all six faces
BEFORE, BBOX = (10, 13, 17), [[1, 9], [2, 12], [1, 15]]
OTHER = (5, 7, 9)                                  # what a resampled axis of a mask case has


def _mask_grid(mask):
    return tuple(OTHER[a] if mask >> a & 1 else E[a] for a in range(3))


# every two-tap mask for both families: the axes of the mask resampled, the others equal (mask 0: the grids agree and the
# member is read as it is, whatever its family), next to a float32 member on the same grid
MASK_CASES = [(f'mask{mask}_{"default" if fam == D else "torch"}',
               [(_mask_grid(mask), (mask + fam) % 2 == 0, fam, None), (E, F32, D, None)], 4, None, BEFORE, BBOX, (0, 1, 2))
              for fam in (D, T) for mask in range(8)]

CASES = MASK_CASES + [
    ('zooms_both_ways', [((5, 7, 6), F16, D, None), ((9, 11, 17), F32, D, None)], 4, None, (9, 12, 15),
     [[1, 8], [2, 11], [1, 14]], (0, 1, 2)),
    ('separate_axis', [((3, 8, 9), F16, D, 0), ((6, 8, 9), F16, D, None), ((4, 7, 11), F32, T, 0)], 4, None, (8, 12, 16),
     [[1, 7], [1, 11], [1, 15]], (0, 1, 2)),
    ('separate_axis_only', [((3, 10, 14), F32, D, 0), ((13, 10, 14), F16, T, 0)], 4, None, BEFORE, BBOX, (0, 1, 2)),
    ('regions_mixed', [((5, 7, 9), F16, D, None), ((11, 13, 10), F32, T, None), (E, F16, T, None), ((4, 10, 9), F32, D, 0)],
     3, [1, 2, 3], BEFORE, BBOX, (1, 2, 0)),
    ('heads61_members5', [((5, 7, 9), F16, D, None), (E, F16, D, None), ((11, 8, 17), F16, T, None), ((4, 5, 7), F32, D, None),
                          ((8, 13, 14), F16, T, 1)], 61, None, BEFORE, BBOX, (0, 1, 2)),
    ('heads300_u16', [((3, 5, 4), F16, D, None), ((5, 4, 9), F16, T, None)], 300, None, (6, 8, 9), [[1, 5], [1, 7], [1, 8]],
     (0, 1, 2)),
    ('heads640_u16_64_threads', [((3, 5, 4), F16, D, None), ((4, 6, 7), F32, T, None)], 640, None, (6, 8, 9),
     [[1, 5], [1, 7], [1, 8]], (2, 0, 1)),
    ('members16', [(((5, 7, 9), F16, D, None), (E, F32, T, None), ((11, 13, 10), F32, T, None), ((8, 7, 14), F16, D, None))[m % 4]
                   for m in range(16)], 4, None, BEFORE, BBOX, (0, 1, 2)),
]


@pytest.mark.parametrize('case', CASES, ids=[c[0] for c in CASES])
def test_fused_equals_resample_then_ensemble_export(case):
    _check(*case)


def test_one_member_on_the_same_grid_is_export_probabilities():
    from test_gpu_ensembling import _export
    for half in (F16, F32):
        for fam in (D, T):
            lgs, avg, labels = _check('same_grid', [(E, half, fam, None)], 4, None, BEFORE, BBOX, (0, 1, 2))
            probs, own = _export(lgs[0], 4, None, BBOX, BEFORE, (0, 1, 2))
            assert torch.equal(avg.view(torch.int32), probs.view(torch.int32)) and torch.equal(labels, own)


PERMS = [(0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)]


@pytest.mark.parametrize('tb', PERMS, ids=[''.join(map(str, tb)) for tb in PERMS])
def test_crop_box_under_every_permutation(tb):
    """Two resampled members on a (5, 6, 7) grid with the box inside on all six faces; outside the box exact 1 / 0 / label 0,
    by the oracle's numpy revert."""
    from oracle import preprocess as opre
    before, bbox = (5, 6, 7), [[1, 4], [2, 5], [1, 6]]
    _, avg, labels = _check('perm', [((2, 4, 3), F16, D, None), ((5, 2, 7), F32, T, None)], 3, None, before, bbox, tb)
    inside = opre.revert_labels(np.ones((3, 3, 5), np.uint8), bbox, before, tb, 4).astype(bool)
    got = avg.cpu().numpy()
    assert (got[0][~inside] == 1).all() and (got[1:][:, ~inside] == 0).all() and not labels.cpu().numpy()[~inside].any()
    assert inside.sum() == 45 and (got[:, inside].sum(0) > 0.99).all()


def test_plateaus_of_the_extreme_fp16_values():
    """A block of the largest finite fp16 and one of the most negative, each spanning several taps of a resampled
    default-family member: fnn_resample clips the blend to the channel's range, the fused pass does not and relies on the
    rounding to fp16 returning the bound itself (the argument at the top of csrc/export_labels.hip)."""
    specs = [((5, 7, 6), F16, D, None), ((9, 11, 17), F16, D, None), ((6, 7, 13), F16, D, 0)]
    lgs = [_member_logits(900 + m, 4, s[0], s[1]) for m, s in enumerate(specs)]
    for lg in lgs:
        lg[0, :3, 2:6] = 65504.0
        lg[1, 1:, :, 3:] = -65504.0
        lg[2, 2] = 65504.0
        lg[3] = -65504.0
        assert torch.isfinite(lg).all()
    _check('plateau', specs, 4, None, (9, 12, 15), [[1, 8], [2, 11], [1, 14]], (0, 1, 2), lgs=lgs)


def test_every_kernel_of_the_file_was_launched():
    """The kernels csrc/ensemble_resample.hip holds, by the build's resource report, against the names
    fnn_op_last_kernels gave after this file's calls."""
    _check('names', [((5, 7, 9), F16, D, None), (E, F32, T, None)], 4, None, BEFORE, BBOX, (0, 1, 2))
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'fast-nnunet_amd', 'csrc')
    report = os.path.join(csrc, 'ensemble_resample.res')
    if not os.path.isfile(report):
        pytest.skip('no resource report: the library was not built by csrc/Makefile here')
    built = set(re.findall(r'Function Name: (\S+)', open(report, errors='replace').read()))
    assert built and len(built) == len(SEEN)
    for mangled in built:
        assert any(re.search(r'\d' + re.escape(name) + r'(E|I)', mangled) for name in SEEN), mangled


# ---------------------------------------------------------------------------------------------------------------
# nnUNetEnsemblePredictor: the fused step against the two-step one and against the members' own exports
# ---------------------------------------------------------------------------------------------------------------
def _raw_case(seed, shape=(34, 40, 52)):
    rng = np.random.default_rng(seed)
    raw = (rng.standard_normal((1, *shape)) * 300 + 150).astype(np.float32)
    raw[:, :3] = 0
    raw[:, :, -2:] = 0
    return raw


def _bits32(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope='module')
def members():
    """The toy members of tests/test_gpu_ensembling.py: 3d_fullres at spacing 1, 3d_lowres at spacing 2."""
    return [_member('3d_fullres', 17), _member('3d_lowres', 29)]


@pytest.mark.parametrize('spacing, resampled', [([1.0, 1.0, 1.0], [False, True]), ([1.0, 0.8, 0.8], [True, True])],
                         ids=['one_member_on_the_grid', 'both_members_resampled'])
def test_ensemble_predictor_fused_equals_two_step_and_the_members_own_exports(members, spacing, resampled):
    from fast_nnunet_amd.ensembling import nnUNetEnsemblePredictor
    from fast_nnunet_amd.preprocess import case_label_export_plan
    raw, props = _raw_case(12), {'spacing': spacing}
    plans = []
    for p in members:
        _, data, pr = p._preprocess_case(raw, dict(props))
        plans.append(case_label_export_plan(data.shape[1:], p.plans_manager, p.configuration_manager, pr)['path'])
    assert plans == ['fused-default' if r else 'same-grid' for r in resampled]
    own = [p.predict_single_npy_array(raw, dict(props), save_or_return_probabilities=True) for p in members]
    want_avg = ensemble_ref.average([pr for _, pr in own])
    want = ensemble_ref.merge_rule(want_avg).astype(np.uint8)
    assert want_avg[0, 0].min() == 1.0                          # cropped away: background probability 1
    assert not np.array_equal(want, own[0][0]) and not np.array_equal(want, own[1][0])   # the ensemble decided something
    fused, two_step = nnUNetEnsemblePredictor(members, fused_export=True), nnUNetEnsemblePredictor(members, fused_export=False)
    results = {}
    for name, ens in (('fused', fused), ('two-step', two_step)):
        got, got_avg = ens.predict_single_npy_array(raw, dict(props), save_or_return_probabilities=True)
        assert got.dtype == np.uint8 and np.array_equal(got, want), name
        assert np.array_equal(_bits32(got_avg), _bits32(want_avg)), name
        assert np.array_equal(ens.predict_single_npy_array(raw, dict(props)), want), name
        results[name] = (got, got_avg)
    assert np.array_equal(results['fused'][0], results['two-step'][0])
    assert np.array_equal(_bits32(results['fused'][1]), _bits32(results['two-step'][1]))
    assert fused.export_stats == {'fused': 2, 'two-step': 0} and two_step.export_stats == {'fused': 0, 'two-step': 2}


def test_ensemble_predictor_postprocesses_the_fused_labels(members, tmp_path):
    from fast_nnunet_amd import postprocessing as pp
    from fast_nnunet_amd.ensembling import nnUNetEnsemblePredictor
    from test_postprocessing_cpu import apply_ref
    raw, props = _raw_case(12), {'spacing': [1.0, 1.0, 1.0]}
    ens = nnUNetEnsemblePredictor(members, fused_export=True)
    want, want_avg = ens.predict_single_npy_array(raw, dict(props), save_or_return_probabilities=True)
    f = pp.remove_all_but_largest_component_from_segmentation
    kwargs = [{'labels_or_regions': [1, 2, 3]}] + [{'labels_or_regions': i} for i in (1, 2, 3)]
    path = tmp_path / 'postprocessing.pkl'
    with open(path, 'wb') as fh:
        pickle.dump(([f] * 4, kwargs), fh)
    ens.set_postprocessing(str(path))
    got_pp, got_pp_avg = ens.predict_single_npy_array(raw, dict(props), save_or_return_probabilities=True)
    assert np.array_equal(got_pp, apply_ref(want, kwargs)) and not np.array_equal(got_pp, want)
    assert np.array_equal(_bits32(got_pp_avg), _bits32(want_avg))
    assert ens.export_stats == {'fused': 2, 'two-step': 0}
    with pytest.raises(NotImplementedError):
        ens.predict_single_npy_array(raw, dict(props), output_file_truncated='x')


# ---------------------------------------------------------------------------------------------------------------
# files
# ---------------------------------------------------------------------------------------------------------------
NOT_RAS = ((2, 0, 1), (1, -1, 1))                  # the orientation of case c1 (the tiled transpose of csrc/reorient.hip)


@pytest.fixture(scope='module')
def files(tmp_path_factory):
    """Three cases - two RAS+ ones written with NiftiIO (one of them at spacing (1, 0.8, 0.8)), one stored in another
    orientation - predicted to files by an ensemble of two NiftiReorientIO members, next to the array route's results."""
    import orient_ref
    from fast_nnunet_amd.ensembling import nnUNetEnsemblePredictor
    from fast_nnunet_amd.imageio import NiftiIO, NiftiReorientIO
    from test_gpu_reorient import _oriented_file
    tmp = tmp_path_factory.mktemp('ensemble_files')
    src, out = tmp / 'in', tmp / 'out'
    src.mkdir()
    mem = [_member('3d_fullres', 17), _member('3d_lowres', 29)]
    for p in mem:
        p.dataset_json['overwrite_image_reader_writer'] = 'NibabelIOWithReorient'
    values = [np.clip(_raw_case(40 + k, (30 + 2 * k, 40, 48))[0], 0, 2000).astype(np.uint16) for k in range(3)]
    for k, zooms in ((0, (1.0, 1.0, 1.0)), (2, (0.8, 0.8, 1.0))):                       # (x, y, z)
        NiftiIO().write_seg(values[k], str(src / f'c{k}_0000.nii.gz'), {'nibabel_stuff': {'original_affine': np.diag([*zooms, 1.0])}})
    _oriented_file(str(src / 'c1_0000.nii.gz'), values[1].astype(np.int16), 4, *NOT_RAS, ras_affine=np.diag([1.0, 1.0, 1.0, 1.0]))
    ens = nnUNetEnsemblePredictor(mem)
    assert isinstance(ens._reader_writer(), NiftiReorientIO)
    returned = ens.predict_from_files(str(src), str(out), save_probabilities=True, num_processes_preprocessing=2,
                                      num_processes_segmentation_export=2)
    arrays = []
    for k in range(3):
        img, props = NiftiReorientIO().read_images([str(src / f'c{k}_0000.nii.gz')], on_device=False)
        arrays.append(ens.predict_single_npy_array(img, props, save_or_return_probabilities=True))
    to_ras = {k: (orient_ref.ornt_of(*NOT_RAS) if k == 1 else None) for k in range(3)}
    return dict(tmp=tmp, src=src, out=out, members=mem, ens=ens, returned=returned, arrays=arrays, to_ras=to_ras)


def _ras_voxels(files, fname, k):
    import nifti_ref
    import orient_ref
    labels = nifti_ref.read(str(fname))[0]
    return labels if files['to_ras'][k] is None else orient_ref.apply_zyx(labels, files['to_ras'][k])


def test_files_hold_the_array_routes_labels_and_a_members_header(files):
    import threading
    import nifti_ref
    from fast_nnunet_amd.ensembling import load_properties_pkl
    out, ens = files['out'], files['ens']
    assert files['returned'] == [None] * 3 and ens.export_stats['two-step'] == 0 and ens.export_stats['fused'] == 6
    assert sorted(os.listdir(out)) == sorted([f'c{k}{e}' for k in range(3) for e in ('.nii.gz', '.npz', '.pkl')] +
                                             ['dataset.json', 'plans.json', 'predict_from_raw_data_args.json'])
    own = files['tmp'] / 'own0'
    assert files['members'][0].predict_from_files(str(files['src']), str(own)) == [None] * 3
    for k in range(3):
        want, want_avg = files['arrays'][k]
        assert len(np.unique(want)) >= 2
        assert np.array_equal(_ras_voxels(files, out / f'c{k}.nii.gz', k), want), k
        assert nifti_ref.file_bytes(out / f'c{k}.nii.gz')[:352] == nifti_ref.file_bytes(own / f'c{k}.nii.gz')[:352], k
        assert np.array_equal(_bits32(np.load(out / f'c{k}.npz')['probabilities']), _bits32(want_avg)), k
        pkl = load_properties_pkl(str(out / f'c{k}.pkl'))
        assert tuple(pkl['shape_before_cropping']) == want.shape[2:] + want.shape[:2] and 'bbox_used_for_cropping' in pkl, k
    assert nifti_ref.read(str(out / 'c1.nii.gz'))[0].shape != files['arrays'][1][0].shape      # c1 is in its file's frame
    assert not [t.name for t in threading.enumerate() if t.name.startswith('fnn-')]


def test_ensemble_folders_on_the_members_own_probabilities_writes_the_same_voxels(files):
    from fast_nnunet_amd.ensembling import ensemble_folders
    folders = []
    for m, p in enumerate(files['members']):
        folders.append(str(files['tmp'] / f'probs{m}'))
        assert p.predict_from_files(str(files['src']), folders[-1], save_probabilities=True) == [None] * 3
    merged = files['tmp'] / 'merged'
    ensemble_folders(folders, str(merged))
    for k in range(3):
        assert np.array_equal(_ras_voxels(files, merged / f'c{k}.nii.gz', k), files['arrays'][k][0]), k


def test_files_without_a_target_parts_overwrite_and_device_compression(files):
    from fast_nnunet_amd.ensembling import nnUNetEnsemblePredictor
    ens, src, out, tmp = files['ens'], str(files['src']), files['out'], files['tmp']
    got = ens.predict_from_files(src, None, save_probabilities=True)
    seq = ens.predict_from_files_sequential(src, None)
    for k in range(3):
        assert np.array_equal(got[k][0], files['arrays'][k][0]) and np.array_equal(seq[k], got[k][0]), k
        assert np.array_equal(_bits32(got[k][1]), _bits32(files['arrays'][k][1])), k
    # num_parts / part_id split the cases
    parts = tmp / 'parts'
    assert ens.predict_from_files(src, str(parts), num_parts=2, part_id=0) == [None] * 2
    assert sorted(f for f in os.listdir(parts) if f.endswith('.nii.gz')) == ['c0.nii.gz', 'c2.nii.gz']
    assert ens.predict_from_files(src, str(parts), num_parts=2, part_id=1) == [None]
    for k in range(3):
        assert open(parts / f'c{k}.nii.gz', 'rb').read() == open(out / f'c{k}.nii.gz', 'rb').read(), k
    # overwrite=False skips finished cases
    assert ens.predict_from_files(src, str(parts), overwrite=False) is None
    os.remove(parts / 'c1.nii.gz')
    before = {k: os.stat(parts / f'c{k}.nii.gz').st_mtime_ns for k in (0, 2)}
    assert ens.predict_from_files(src, str(parts), overwrite=False) == [None]
    assert open(parts / 'c1.nii.gz', 'rb').read() == open(out / 'c1.nii.gz', 'rb').read()
    assert before == {k: os.stat(parts / f'c{k}.nii.gz').st_mtime_ns for k in (0, 2)}
    # compress_on_device: another deflate stream around the same bytes
    on_device = nnUNetEnsemblePredictor(files['members'], compress_on_device=True)
    packed = tmp / 'packed'
    assert on_device.predict_from_files_sequential(src, str(packed)) == [None] * 3
    for k in range(3):
        assert gzip.open(packed / f'c{k}.nii.gz', 'rb').read() == gzip.open(out / f'c{k}.nii.gz', 'rb').read(), k
    assert open(packed / 'c0.nii.gz', 'rb').read() != open(out / 'c0.nii.gz', 'rb').read()
