"""Cross-configuration ensembling on a real MI355X (fnn_ensemble_export / fnn_average_probabilities, csrc/ensemble.hip):
every member's probabilities must be bit for bit what fnn_export_probabilities writes for it, the average bit for bit
numpy's float32 average_probabilities, the labels the reference's merge rule on that average; then the .npz route
against the reference-made golden, nnUNetEnsemblePredictor end to end, and a 61-head 256^3 case."""
import os
import pickle

import numpy as np
import pytest
import torch

import ensemble_ref

pytestmark = pytest.mark.gpu

F16, F32 = True, False


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _member_logits(seed, heads, cropped, half):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((heads, *cropped), generator=g) * 3
    x[:, 0, 0, :3] = x[0, 0, 0, 0]                # every head equal: an exact tie of all heads in every member
    x[1, 1] = x[0, 1]                             # heads 0 and 1 tied along a plane
    return x.to(torch.half if half else torch.float32).cuda().contiguous()


def _export(lg, heads, order, bbox, before, tb, u16=False):
    from fast_nnunet_amd import capi
    grid = [before[j] for j in tb]
    probs = torch.empty((heads, *grid), dtype=torch.float32, device='cuda')
    labels = torch.empty(grid, dtype=torch.int16 if u16 else torch.uint8, device='cuda')
    capi.export_probabilities(lg.data_ptr(), lg.dtype == torch.half, heads, order, bbox, before, tb, probs.data_ptr(),
                              labels.data_ptr(), u16, _stream())
    return probs, labels


def _ensemble(lgs, heads, order, bbox, before, tb, u16=False, with_avg=True):
    from fast_nnunet_amd import capi
    grid = [before[j] for j in tb]
    avg = torch.empty((heads, *grid), dtype=torch.float32, device='cuda') if with_avg else None
    labels = torch.empty(grid, dtype=torch.int16 if u16 else torch.uint8, device='cuda')
    capi.ensemble_export([lg.data_ptr() for lg in lgs], [lg.dtype == torch.half for lg in lgs], heads, order, bbox,
                         before, tb, None if avg is None else avg.data_ptr(), labels.data_ptr(), u16, _stream())
    return avg, labels


def _labels_np(t, u16):
    a = t.cpu().numpy()
    return a.view(np.uint16).astype(np.int64) if u16 else a.astype(np.int64)


# (n members, member dtypes, heads, regions_class_order, shape_before_cropping (transposed axes), bbox, transpose_backward)
KERNEL_CASES = [
    ('n1_identity_vec', 1, [F16], 4, None, (12, 16, 20), [[1, 9], [2, 14], [4, 16]], (0, 1, 2)),
    ('n2_f32_transposed', 2, [F32, F32], 2, None, (11, 13, 9), [[1, 10], [2, 12], [1, 8]], (2, 0, 1)),
    ('n3_mixed_regions', 3, [F16, F32, F16], 3, [1, 2, 3], (10, 12, 14), [[2, 9], [1, 11], [3, 12]], (1, 2, 0)),
    ('n5_61_heads_vec', 5, [F16] * 5, 61, None, (9, 10, 24), [[1, 8], [0, 10], [4, 20]], (0, 1, 2)),
    ('n16_mixed', 16, [F16, F32] * 8, 4, None, (8, 9, 12), [[1, 7], [1, 8], [0, 12]], (0, 1, 2)),
    ('n2_300_heads_u16', 2, [F16, F16], 300, None, (6, 7, 8), [[1, 5], [0, 7], [2, 7]], (0, 1, 2)),
    ('n2_regions_unaligned', 2, [F16, F32], 3, [1, 2, 3], (7, 9, 13), [[0, 7], [1, 8], [3, 10]], (0, 1, 2)),
    ('n1_regions_transposed', 1, [F32], 3, [2, 1, 3], (9, 8, 7), [[1, 8], [1, 7], [0, 7]], (2, 1, 0)),
]


# The crop-box map (fnn_device.h, crop_box_voxel) under all six permutations: a grid of three different extents, none a
# multiple of 4, the box inside on all six faces; then the identity transpose with the z box on multiples of 4 (the VEC = 4
# kernel) and the same case with lo[2] = 3 (VEC = 1).  Two members each, so that the average is not one member's export.
CROP_MAP_CASES = [(f'perm_{"".join(map(str, tb))}', 2, [F16, F32], 3, None, (5, 6, 7), [[1, 4], [2, 5], [1, 6]], tb)
                  for tb in [(0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)]] + [
    ('z_box_4_to_8_vec4', 2, [F16, F32], 3, None, (3, 5, 8), [[1, 3], [1, 4], [4, 8]], (0, 1, 2)),
    ('z_box_3_to_7_vec1', 2, [F16, F32], 3, None, (3, 5, 8), [[1, 3], [1, 4], [3, 7]], (0, 1, 2)),
]


@pytest.mark.parametrize('case', CROP_MAP_CASES, ids=[c[0] for c in CROP_MAP_CASES])
def test_ensemble_export_puts_the_box_where_the_oracle_puts_it(case):
    """The export kernel shares the map, so the comparison below cannot see a map that is wrong in both: here the voxels
    come from the oracle's numpy revert - exact 1 / 0 / label 0 outside the box; inside, each member within the 5e-7 of
    test_gpu_preprocess's export rule, so their average within that plus the two roundings (half an ulp of 1 each) of + and /."""
    from oracle import preprocess as opre
    name, n, dtypes, heads, order, before, bbox, tb = case
    cropped = [hi - lo for lo, hi in bbox]
    lgs = [_member_logits(100 * len(name) + m, heads, cropped, dtypes[m]) for m in range(n)]
    refs = [opre.export_with_probabilities(lg.cpu().numpy(), bbox, before, tb, 4)[1] for lg in lgs]
    inside = opre.revert_labels(np.ones(cropped, np.uint8), bbox, before, tb, 4).astype(bool)
    avg, labels = _ensemble(lgs, heads, order, bbox, before, tb)
    got, want = avg.cpu().numpy(), ensemble_ref.average(refs)
    assert np.array_equal(got[:, ~inside].view(np.uint32), want[:, ~inside].view(np.uint32)), name
    assert not _labels_np(labels, False)[~inside].any(), name
    assert np.abs(got - want).max() <= 5e-7 + 2 * 2.0 ** -24, name


@pytest.mark.parametrize('case', KERNEL_CASES + CROP_MAP_CASES, ids=[c[0] for c in KERNEL_CASES + CROP_MAP_CASES])
def test_ensemble_export_equals_per_member_export_and_numpy_average(case):
    name, n, dtypes, heads, order, before, bbox, tb = case
    u16 = heads > 255
    cropped = [hi - lo for lo, hi in bbox]
    lgs = [_member_logits(100 * len(name) + m, heads, cropped, dtypes[m]) for m in range(n)]
    members = [_export(lg, heads, order, bbox, before, tb, u16) for lg in lgs]
    probs = [p.cpu().numpy() for p, _ in members]
    want_avg = ensemble_ref.average(probs)
    want_labels = ensemble_ref.merge_rule(want_avg, order).astype(np.int64)
    avg, labels = _ensemble(lgs, heads, order, bbox, before, tb, u16)
    got_avg = avg.cpu().numpy()
    assert np.array_equal(got_avg.view(np.uint32), want_avg.view(np.uint32)), name
    assert np.array_equal(_labels_np(labels, u16), want_labels), name
    _, labels_only = _ensemble(lgs, heads, order, bbox, before, tb, u16, with_avg=False)
    assert torch.equal(labels_only, labels), name
    if n == 1:
        assert torch.equal(avg, members[0][0]), name
        if order is None:
            assert torch.equal(labels, members[0][1]), name
    if order is None:                                       # the crafted ties are decided by the first maximum
        assert (want_labels == 0).any()


def test_average_probabilities_matches_reference_golden(golden_dir, tmp_path):
    from fast_nnunet_amd import ensembling
    from fast_nnunet_amd.plans import LabelManager
    from golden_cases import DATASET_JSONS
    z = np.load(os.path.join(golden_dir, 'ensemble.npz'))
    for name, (dataset, n) in {'labels_2_transposed': ('two_mod', 2), 'labels_4_crop': ('labels3', 4),
                               'regions_3_crop': ('regions', 3)}.items():
        members = [z[f'{name}__member{m}'] for m in range(n)]
        files = []
        for m, p in enumerate(members):
            files.append(str(tmp_path / f'{name}_{m}.npz'))
            np.savez_compressed(files[-1], probabilities=p)
        ref_avg, ref_seg = z[name + '__avg'], z[name + '__seg']
        assert np.array_equal(ensembling.average_probabilities(files).view(np.uint32), ref_avg.view(np.uint32)), name
        dj = DATASET_JSONS[dataset]
        lm = LabelManager(dj['labels'], dj.get('regions_class_order'))
        seg, avg = ensembling.ensemble_probabilities(members, lm, return_probabilities=True)
        assert np.array_equal(avg.view(np.uint32), ref_avg.view(np.uint32)), name
        assert np.array_equal(ensembling.ensemble_probabilities(files, lm), seg), name
        if lm.has_regions:
            decided = ((ref_avg > 4e-6) | (ref_avg == 0)).all(0)
        else:
            top2 = np.sort(ref_avg, 0)[-2:]
            decided = (top2[1] - top2[0] > 1e-6) | (top2[1] == top2[0])
        assert decided.mean() > 0.99 and np.array_equal(seg[decided].astype(np.int64), ref_seg[decided].astype(np.int64)), name


def _member(configuration, seed, heads=4, transpose_forward=(2, 0, 1)):
    from fast_nnunet_amd import nnUNetPredictor
    from fast_nnunet_amd.plans import PlansManager
    from golden_cases import toy_unet_spec
    from oracle.unet import synthetic_state_dict
    spec = toy_unet_spec(1, heads)
    ip = {'0': {'mean': 100.0, 'std': 250.0, 'percentile_00_5': -400.0, 'percentile_99_5': 800.0}}
    conf = {'normalization_schemes': ['CTNormalization'], 'use_mask_for_norm': [False],
            'architecture': {'network_class_name': 'PlainConvUNet', 'arch_kwargs': {}, '_kw_requires_import': []}}
    tf = list(transpose_forward)
    pm = PlansManager({'dataset_name': 'Dataset996_Ensemble', 'plans_name': 'nnUNetPlans', 'transpose_forward': tf,
                       'transpose_backward': [int(i) for i in np.argsort(tf)],
                       'foreground_intensity_properties_per_channel': ip,
                       'configurations': {'3d_fullres': dict(conf, patch_size=[16, 16, 32], spacing=[1.0, 1.0, 1.0]),
                                          '3d_lowres': dict(conf, patch_size=[16, 16, 16], spacing=[2.0, 2.0, 2.0])}})
    dj = {'labels': {('background' if i == 0 else f'c{i}'): i for i in range(heads)}, 'channel_names': {'0': 'CT'},
          'file_ending': '.nii.gz'}
    p = nnUNetPredictor(tile_step_size=0.5, use_gaussian=True, use_mirroring=False, perform_everything_on_device=True,
                        device=torch.device('cuda', 0), verbose=False, allow_tqdm=False, patches_per_forward=3)
    p.manual_initialization(None, pm, pm.get_configuration(configuration), [synthetic_state_dict(spec, seed)], dj,
                            'nnUNetTrainer', None)
    return p


def test_ensemble_predictor_end_to_end(tmp_path):
    from fast_nnunet_amd import postprocessing as pp
    from fast_nnunet_amd.ensembling import nnUNetEnsemblePredictor
    from test_postprocessing_cpu import apply_ref
    members = [_member('3d_fullres', 17), _member('3d_lowres', 29)]
    ens = nnUNetEnsemblePredictor(members)
    rng = np.random.default_rng(12)
    raw = (rng.standard_normal((1, 34, 40, 52)) * 300 + 150).astype(np.float32)
    raw[:, :3] = 0
    raw[:, :, -2:] = 0
    props = {'spacing': [1.0, 1.0, 1.0]}
    own = [p.predict_single_npy_array(raw, dict(props), save_or_return_probabilities=True) for p in members]
    want_avg = ensemble_ref.average([pr for _, pr in own])
    want = ensemble_ref.merge_rule(want_avg).astype(np.uint8)
    assert want_avg[0, 0].min() == 1.0                          # cropped away: background probability 1
    got, got_avg = ens.predict_single_npy_array(raw, dict(props), save_or_return_probabilities=True)
    assert got.dtype == np.uint8 and np.array_equal(got, want)
    assert np.array_equal(got_avg.view(np.uint32), want_avg.view(np.uint32))
    assert np.array_equal(ens.predict_single_npy_array(raw, dict(props)), want)
    assert not np.array_equal(want, own[0][0]) and not np.array_equal(want, own[1][0])   # the ensemble decided something
    f = pp.remove_all_but_largest_component_from_segmentation
    kwargs = [{'labels_or_regions': [1, 2, 3]}] + [{'labels_or_regions': i} for i in (1, 2, 3)]
    path = tmp_path / 'postprocessing.pkl'
    with open(path, 'wb') as fh:
        pickle.dump(([f] * 4, kwargs), fh)
    ens.set_postprocessing(str(path))
    got_pp, got_pp_avg = ens.predict_single_npy_array(raw, dict(props), save_or_return_probabilities=True)
    assert np.array_equal(got_pp, apply_ref(want, kwargs)) and not np.array_equal(got_pp, want)
    assert np.array_equal(got_pp_avg.view(np.uint32), want_avg.view(np.uint32))
    with pytest.raises(NotImplementedError):
        ens.predict_single_npy_array(raw, dict(props), output_file_truncated='x')


def test_ensemble_predictor_refuses_mismatched_members():
    from fast_nnunet_amd.ensembling import nnUNetEnsemblePredictor
    a = _member('3d_fullres', 17)
    with pytest.raises(ValueError):
        nnUNetEnsemblePredictor([a, _member('3d_lowres', 29, heads=3)])              # other labels
    with pytest.raises(ValueError):
        nnUNetEnsemblePredictor([a, _member('3d_lowres', 29, transpose_forward=(0, 1, 2))])
    with pytest.raises(ValueError):
        nnUNetEnsemblePredictor([a] * 17)


def test_61_heads_256_cube_two_members():
    """Size: 61 heads on a 256^3 raw grid (crop = grid, fp16 logits), against the per-member export averaged by torch on
    the GPU in member order (float32 additions and one division: exact IEEE operations) and torch's argmax."""
    heads, s = 61, 256
    bbox, before, tb = [[0, s]] * 3, (s, s, s), (0, 1, 2)
    lgs = []
    for m in range(2):
        g = torch.Generator(device='cuda').manual_seed(600 + m)
        lgs.append((torch.randn((heads, s, s, s), generator=g, device='cuda') * 3).half())
    avg, labels = _ensemble(lgs, heads, None, bbox, before, tb)
    want = None
    for lg in lgs:
        p, _ = _export(lg, heads, None, bbox, before, tb)
        want = p if want is None else want.add_(p)
        del p
    want.div_(2.0)
    assert torch.equal(avg.view(torch.int32), want.view(torch.int32))
    assert torch.equal(labels.long(), torch.argmax(want, 0))
    _, labels_only = _ensemble(lgs, heads, None, bbox, before, tb, with_avg=False)
    assert torch.equal(labels_only, labels)
