"""Connected-component postprocessing on a real MI355X (fnn_keep_largest_components, csrc/postprocess.hip): the device
result must be bit-identical to the scipy restatement of the reference's rule (tests/test_postprocessing_cpu.py) on
hand-made cases, both label dtypes, shapes that are not tile multiples, components that cross every tile, the
checkerboard, all-tied singletons, random maps near the percolation density, the all-foreground volume, overlapping
regions, a 512^3 61-label map through a whole-foreground plus per-label pkl, and end to end through
``predict_single_npy_array``."""
import numpy as np
import pytest
import torch
from scipy import ndimage

from test_postprocessing_cpu import apply_ref, hand_cases, keep_largest_ref, keep_largest_ref_boxed

pytestmark = pytest.mark.gpu


def _pp():
    from fast_nnunet_amd import postprocessing as pp
    return pp


def _check(seg, lor, bg=0):
    pp = _pp()
    before = seg.copy()
    got = pp.remove_all_but_largest_component_from_segmentation(seg, lor, bg)
    want = keep_largest_ref(seg, lor, bg)
    assert np.array_equal(seg, before)
    assert got.dtype == seg.dtype and got.shape == seg.shape
    bad = np.argwhere(got != want)
    assert bad.size == 0, f'{len(bad)} voxels differ, first {bad[:5].tolist()}'
    return got


@pytest.mark.parametrize('case', hand_cases(), ids=lambda c: c[0])
def test_hand_made_cases(case):
    _, seg, lor, bg, want = case
    got = _check(seg, lor, bg)
    assert np.array_equal(got, want)


@pytest.mark.parametrize('dtype', [np.uint8, np.uint16])
@pytest.mark.parametrize('shape', [(1, 37, 53), (1, 300, 7), (37, 41, 43), (5, 64, 33), (9, 17, 130)])
def test_random_maps_near_percolation(dtype, shape):
    """Site percolation on the 26-neighbour lattice sets in near p = 0.097: around it the components are of every size
    and wind through many tiles."""
    rng = np.random.default_rng(sum(shape) * (2 if dtype == np.uint16 else 1))
    for p in (0.08, 0.1, 0.2):
        mask = rng.random(shape) < p
        seg = np.zeros(shape, dtype)
        if dtype == np.uint8:
            seg[mask] = 1
            _check(seg, [1])
        else:
            seg[mask] = rng.integers(1, 301, int(mask.sum()))
            _check(seg, list(range(1, 301)))                  # the whole foreground, labels above 255
            _check(seg, [(257, 258, 259)], bg=1000)


def test_uint16_labels_above_255_and_int32_device_tensors():
    pp = _pp()
    rng = np.random.default_rng(1)
    seg = rng.integers(0, 3, (20, 21, 22)).astype(np.uint16) * 400
    _check(seg, [400])
    _check(seg, [(400, 800)], bg=65535)
    t = torch.from_numpy(seg.astype(np.int32)).cuda()
    got = pp.remove_all_but_largest_component_from_segmentation(t, [800])
    assert got.dtype == torch.int32 and got.device == t.device and got.data_ptr() != t.data_ptr()
    assert np.array_equal(got.cpu().numpy(), keep_largest_ref(seg.astype(np.int32), [800]))
    t8 = torch.from_numpy((seg // 400).astype(np.uint8)).cuda()
    got8 = pp.remove_all_but_largest_component_from_segmentation(t8, 1)
    assert got8.dtype == torch.uint8 and np.array_equal(got8.cpu().numpy(), keep_largest_ref((seg // 400).astype(np.uint8), 1))
    with pytest.raises(ValueError):
        pp.remove_all_but_largest_component_from_segmentation(torch.full((2, 2, 2), 70000, dtype=torch.int32).cuda(), 1)


def test_serpentine_component_crossing_every_tile():
    """Lines along z through every tile, joined at alternating ends and between planes into one component, plus one
    isolated voxel of debris."""
    X, Y, Z = 24, 40, 80
    zl = Z - 10                                               # the lines end here; debris beyond
    seg = np.zeros((X, Y, Z), np.uint8)
    for x in range(0, X, 2):
        for y in range(0, Y, 2):
            seg[x, y, :zl] = 1
            if y + 2 < Y:
                seg[x, y:y + 3, zl - 1 if (y // 2) % 2 == 0 else 0] = 1
        if x + 2 < X:
            seg[x:x + 3, 0, 0] = 1
    seg[X // 2, Y // 2, Z - 3] = 1
    assert ndimage.label(seg > 0, structure=np.ones((3, 3, 3)))[1] == 2
    got = _check(seg, [1])
    assert got[X // 2, Y // 2, Z - 3] == 0 and got.sum() == seg.sum() - 1


def test_checkerboard_is_one_component_per_parity():
    x, y, z = np.indices((19, 33, 35))
    parity = (x + y + z) % 2
    seg = (parity + 1).astype(np.uint8)                      # labels 1 and 2: each one 26-connected component
    got = _check(seg, [1])
    assert np.array_equal(got, seg)
    _check(seg, [1, 2])                                       # both parities: one component
    got = _check(seg, [2], bg=1)
    assert np.array_equal(got, seg)


def test_all_even_coordinates_are_tied_singletons():
    x, y, z = np.indices((16, 34, 40))
    seg = ((x % 2 == 0) & (y % 2 == 0) & (z % 2 == 0)).astype(np.uint8)
    got = _check(seg, [1])
    assert np.array_equal(got, seg)                           # N/8 singletons, all tied, all kept


def test_all_foreground_hot_root():
    seg = np.ones((64, 96, 128), np.uint8)
    got = _check(seg, [1])
    assert np.array_equal(got, seg)
    seg[10:20, 10:20, 10:20] = 0
    seg[14, 14, 14] = 1                                       # an island inside a hole
    got = _check(seg, [1])
    assert got[14, 14, 14] == 0


def test_overlapping_regions_sequentially_and_fused_passes():
    pp = _pp()
    rng = np.random.default_rng(5)
    seg = rng.integers(0, 4, (30, 31, 33)).astype(np.uint8)
    seg[rng.random(seg.shape) < 0.7] = 0
    f = pp.remove_all_but_largest_component_from_segmentation
    for kwargs in ([{'labels_or_regions': [(1, 2, 3)]}, {'labels_or_regions': [(2, 3)]}, {'labels_or_regions': [3]}],
                   [{'labels_or_regions': [1, 2, 3]}] + [{'labels_or_regions': i} for i in (1, 2, 3)],
                   [{'labels_or_regions': 1, 'background_label': 3}, {'labels_or_regions': 2, 'background_label': 3},
                    {'labels_or_regions': [(3, 0)]}]):
        got = pp.apply_postprocessing(seg, [f] * len(kwargs), kwargs)
        assert np.array_equal(got, apply_ref(seg, kwargs))
        t = torch.from_numpy(seg).cuda()
        got_t = pp.apply_postprocessing(t, [f] * len(kwargs), kwargs)
        assert got_t.is_cuda and np.array_equal(got_t.cpu().numpy(), apply_ref(seg, kwargs))


def test_foreign_callables_run_in_order():
    pp = _pp()
    seg = np.zeros((8, 8, 8), np.uint8)
    seg[0, 0, 0] = 1; seg[4:6, 4:6, 4:6] = 1; seg[7, 7, 0] = 2

    def relabel(s, src, dst):
        s = np.copy(s); s[s == src] = dst
        return s
    f = pp.remove_all_but_largest_component_from_segmentation
    got = pp.apply_postprocessing(seg, [f, relabel, f], [{'labels_or_regions': 1}, {'src': 2, 'dst': 1},
                                                         {'labels_or_regions': 1}])
    want = keep_largest_ref(relabel(keep_largest_ref(seg, 1), 2, 1), 1)
    assert np.array_equal(got, want)


def test_removed_counts_per_set():
    from fast_nnunet_amd import capi
    seg = np.zeros((10, 10, 10), np.uint8)
    seg[0:3, 0:3, 0:3] = 1; seg[8, 8, 8] = 1; seg[5, 0, 9] = 1
    seg[0, 9, 0:4] = 2; seg[9, 0, 0:2] = 2
    t = torch.from_numpy(seg).cuda()
    removed = capi.keep_largest_components(t.data_ptr(), False, t.shape, np.array([-1, 0, 1], np.int32), 2, 0,
                                           torch.cuda.current_stream().cuda_stream)
    assert removed.tolist() == [2, 2]
    want = seg.copy()
    want[8, 8, 8] = 0; want[5, 0, 9] = 0; want[9, 0, 0:2] = 0
    assert np.array_equal(t.cpu().numpy(), want)


def test_512_cube_61_labels_whole_foreground_plus_per_label_pkl():
    pp = _pp()
    rng = np.random.default_rng(61)
    n = 512
    # blobs: smoothed noise cut into 60 bands above a threshold, so every label has large bodies and debris
    small = ndimage.gaussian_filter(rng.standard_normal((n // 8,) * 3).astype(np.float32), 1.0)
    field = ndimage.zoom(small, 8, order=1)
    seg = np.clip((field - 0.1) * 150, 0, 60).astype(np.uint8)
    seg[(field > 0.1) & (seg == 0)] = 1
    del field
    idx = rng.integers(0, seg.size, 20000)
    seg.reshape(-1)[idx] = rng.integers(1, 61, idx.size).astype(np.uint8)
    labels = list(range(1, 61))
    kwargs = [{'labels_or_regions': labels}] + [{'labels_or_regions': i} for i in labels]
    f = pp.remove_all_but_largest_component_from_segmentation
    assert len(pp.plan_passes([f] * len(kwargs), kwargs)) == 2
    got = pp.apply_postprocessing(seg, [f] * len(kwargs), kwargs)
    want = keep_largest_ref(seg, labels)
    boxes = ndimage.find_objects(want)
    for lab in labels:
        if lab - 1 < len(boxes) and boxes[lab - 1] is not None:
            want = keep_largest_ref_boxed(want, lab, 0, boxes[lab - 1])
    assert np.array_equal(got, want), int((got != want).sum())


def _raw_case():
    from fast_nnunet_amd import nnUNetPredictor
    from fast_nnunet_amd.plans import PlansManager
    from golden_cases import toy_unet_spec
    from oracle.unet import synthetic_state_dict
    heads = 4
    spec, patch = toy_unet_spec(1, heads), (16, 16, 32)
    ip = {'0': {'mean': 100.0, 'std': 250.0, 'percentile_00_5': -400.0, 'percentile_99_5': 800.0}}
    pm = PlansManager({'dataset_name': 'Dataset999_Golden', 'plans_name': 'nnUNetPlans', 'transpose_forward': [0, 1, 2],
                       'transpose_backward': [0, 1, 2], 'foreground_intensity_properties_per_channel': ip,
                       'configurations': {'3d_fullres': {
                           'patch_size': list(patch), 'spacing': [1.0, 1.0, 1.0], 'normalization_schemes': ['CTNormalization'],
                           'use_mask_for_norm': [False],
                           'architecture': {'network_class_name': 'PlainConvUNet', 'arch_kwargs': {}, '_kw_requires_import': []}}}})
    dj = {'labels': {('background' if i == 0 else f'c{i}'): i for i in range(heads)}, 'channel_names': {'0': 'CT'},
          'file_ending': '.nii.gz'}
    p = nnUNetPredictor(tile_step_size=0.5, use_gaussian=True, use_mirroring=False, perform_everything_on_device=True,
                        device=torch.device('cuda', 0), verbose=False, allow_tqdm=False, patches_per_forward=3)
    p.manual_initialization(None, pm, pm.get_configuration('3d_fullres'), [synthetic_state_dict(spec, 17)], dj,
                            'nnUNetTrainer', None)
    return p


@pytest.mark.parametrize('spacing', [(1.0, 1.0, 1.0), (1.5, 0.8, 0.8)])        # same grid; resampled
def test_predict_single_npy_array_with_postprocessing(spacing, tmp_path):
    import pickle
    pp = _pp()
    p = _raw_case()
    rng = np.random.default_rng(11)
    raw = (rng.standard_normal((1, 34, 40, 52)) * 300 + 150).astype(np.float32)
    raw[:, :3] = 0
    props = {'spacing': list(spacing)}
    plain = p.predict_single_npy_array(raw, dict(props))
    plain_seg, plain_probs = p.predict_single_npy_array(raw, dict(props), save_or_return_probabilities=True)
    f = pp.remove_all_but_largest_component_from_segmentation
    kwargs = [{'labels_or_regions': [1, 2, 3]}] + [{'labels_or_regions': i} for i in (1, 2, 3)]
    path = tmp_path / 'postprocessing.pkl'
    with open(path, 'wb') as fh:
        pickle.dump(([f] * 4, kwargs), fh)
    p.set_postprocessing(str(path))
    got = p.predict_single_npy_array(raw, dict(props))
    got_seg, got_probs = p.predict_single_npy_array(raw, dict(props), save_or_return_probabilities=True)
    assert got.dtype == plain.dtype and got.shape == plain.shape
    assert np.array_equal(got, apply_ref(plain, kwargs))
    assert np.array_equal(got_seg, apply_ref(plain_seg, kwargs))
    assert np.array_equal(got_probs, plain_probs)
    assert not np.array_equal(got, plain)                    # the postprocessing did something on this case
    p.set_postprocessing(None)
    assert np.array_equal(p.predict_single_npy_array(raw, dict(props)), plain)
