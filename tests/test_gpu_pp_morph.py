"""Small-component removal and hole filling on a real MI355X (fnn_remove_small_components, fnn_fill_holes,
csrc/postprocess.hip; the labelling with face connectivity, csrc/cc_label.h): every device result must equal the scipy
restatement of tests/pp_morph_ref.py exactly - hand-made maps, shapes that are no multiple of the 1024-voxel tile with
components and holes across the tile faces of every axis, both label dtypes, labels at and beyond the table, other
backgrounds, 2-D maps, empty and full sets, the counts the entries return, and the front ends."""

import numpy as np
import pytest
import torch
from scipy import ndimage

import pp_morph_ref as ref

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda', 0)
SHAPES = [(19, 21, 37), (33, 5, 130)]                       # tiles of 8 x 8 x 16 and a thin middle axis


def _pp():
    from fast_nnunet_amd import postprocessing as pp
    return pp


def _same(got, want, seg):
    assert got.dtype == seg.dtype and got.shape == seg.shape
    bad = np.argwhere(got != want)
    assert bad.size == 0, f'{len(bad)} voxels differ, first {bad[:5].tolist()}: got {got[tuple(bad[0])]}, want {want[tuple(bad[0])]}'


def _check_small(seg, **kw):
    before = seg.copy()
    got = _pp().remove_small_components_from_segmentation(seg, **kw)
    assert np.array_equal(seg, before)
    _same(got, ref.remove_small_ref(seg, **kw), seg)
    return got


def _check_holes(seg, **kw):
    before = seg.copy()
    got = _pp().fill_holes_in_segmentation(seg, **kw)
    assert np.array_equal(seg, before)
    _same(got, ref.fill_holes_ref(seg, **kw), seg)
    return got


def _entry_small(seg, table, n_groups, min_size, connectivity, bg=0):
    """The C entry on a copy of ``seg`` (uint8 / uint16): (result, removed per set)."""
    from fast_nnunet_amd import capi
    u16 = seg.dtype == np.uint16
    t = torch.from_numpy(seg.astype(np.int16) if u16 else seg.copy()).to(DEV)
    removed = capi.remove_small_components(t.data_ptr(), u16, t.shape, table, n_groups, bg, min_size, connectivity)
    return t.cpu().numpy().view(seg.dtype), removed


def _entry_holes(seg, table, bg, fill, border_axes):
    from fast_nnunet_amd import capi
    u16 = seg.dtype == np.uint16
    t = torch.from_numpy(seg.astype(np.int16) if u16 else seg.copy()).to(DEV)
    filled = capi.fill_holes(t.data_ptr(), u16, t.shape, table, bg, fill, border_axes)
    return t.cpu().numpy().view(seg.dtype), filled


def _blobs(shape, n_labels, seed, sigma=1.5, dtype=np.uint8, level=0.52):
    """Thresholded smoothed noise, its foreground split into labels by a second smooth field: components of every size,
    cavities, and many label borders."""
    rng = np.random.default_rng(seed)
    a = ndimage.gaussian_filter(rng.random(shape), sigma, mode='constant', cval=0.5)
    b = ndimage.gaussian_filter(rng.random(shape), 2 * sigma, mode='wrap')
    rank = (np.argsort(np.argsort(b.ravel())).reshape(shape) * n_labels) // b.size
    seg = np.where(a > np.quantile(a, level), rank + 1, 0)
    return seg.astype(dtype)


@pytest.fixture(scope='module')
def noise96():
    return _blobs((96, 96, 96), 12, seed=34, sigma=1.0, level=0.4)


# ---- hand-made maps ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', ref.hole_cases(), ids=lambda c: c[0])
def test_hole_hand_made_maps(case):
    _, seg, kw, want = case
    assert np.array_equal(_check_holes(seg, **kw), want)


@pytest.mark.parametrize('case', ref.small_cases(), ids=lambda c: c[0])
def test_small_component_hand_made_maps(case):
    _, seg, kw, want = case
    assert np.array_equal(_check_small(seg, **kw), want)


# ---- geometry ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('connectivity', [6, 26])
@pytest.mark.parametrize('shape', SHAPES)
def test_small_components_across_tile_faces(shape, connectivity):
    """Thin lines along each axis through several tiles (one component however many tiles it crosses), diagonal steps at the
    tile faces (joined at 26, apart at 6), and random maps around the percolation densities of both lattices."""
    seg = np.zeros(shape, np.uint8)
    seg[1, 1, :] = 1; seg[:, 2, 3] = 1; seg[3, :, 5] = 1      # lines along z, x, y; they do not touch each other
    for k in range(min(shape) - 1):                           # a staircase of corner contacts through the volume
        seg[k, min(k, shape[1] - 1), 20 + (k % 2)] = 2
    for m in (2, shape[2], shape[2] + 1, 10 ** 6):
        _check_small(seg, labels_or_regions=[1, 2], min_size=m, connectivity=connectivity, per_member=True)
    rng = np.random.default_rng(sum(shape) + connectivity)
    for p in (0.1, 0.25, 0.35):
        seg = (rng.random(shape) < p).astype(np.uint8) * rng.integers(1, 4, shape).astype(np.uint8)
        _check_small(seg, labels_or_regions=[1, 2, 3], min_size=6, connectivity=connectivity)
        _check_small(seg, labels_or_regions=[1, (2, 3)], min_size=[3, 40], connectivity=connectivity, per_member=True, background_label=9)


@pytest.mark.parametrize('shape', SHAPES)
def test_holes_across_tile_faces(shape):
    """A thick-walled box whose cavity spans several tiles in every axis, closed; then opened by a tunnel; cavities in random
    blobs; a set whose complement is a maze (dense random mask)."""
    seg = np.zeros(shape, np.uint8)
    X, Y, Z = shape
    seg[1:X - 1, 1:Y - 1, 1:Z - 1] = 1
    seg[2:X - 2, 2:Y - 2, 2:Z - 2] = 0
    seg[X // 2, Y // 2, Z // 2] = 3                           # a foreign label inside the cavity stays
    got = _check_holes(seg, labels_or_regions=[1])
    assert got[2, 2, 2] == 1 and got[X // 2, Y // 2, Z // 2] == 3
    seg[X - 2, Y // 2, Z // 2] = 0                            # a one-voxel tunnel
    got = _check_holes(seg, labels_or_regions=[1])
    assert np.array_equal(got, seg)
    rng = np.random.default_rng(sum(shape))
    for p in (0.5, 0.7, 0.8):                                 # face-connected complements break up near 1 - 0.31
        seg = (rng.random(shape) < p).astype(np.uint8)
        _check_holes(seg, labels_or_regions=[1])
    seg = _blobs(shape, 3, seed=7)
    for lab in (1, 2, 3):
        _check_holes(seg, labels_or_regions=[lab])
    _check_holes(seg, labels_or_regions=[(1, 2, 3)], fill_label=2)


def test_two_by_two_by_two_and_zero_size_volumes():
    seg = np.array([[[1, 0], [0, 1]], [[0, 1], [1, 0]]], np.uint8)          # four voxels that touch at edges only
    assert np.array_equal(_check_small(seg, labels_or_regions=[1], min_size=4, connectivity=26), seg)
    assert not _check_small(seg, labels_or_regions=[1], min_size=4, connectivity=6).any()
    assert np.array_equal(_check_holes(seg, labels_or_regions=[1]), seg)
    for shape in ((0, 4, 5), (3, 0, 5), (3, 4, 0)):
        empty = np.zeros(shape, np.uint8)
        assert _pp().remove_small_components_from_segmentation(empty, [1], 5).shape == shape
        assert _pp().fill_holes_in_segmentation(empty, [1]).shape == shape


def test_two_d_map_and_the_depth_one_volume_with_both_border_masks():
    """(33, 65) as a 2-D map: scipy on the 2-D array.  The entry on [1, Y, Z]: border_axes 6 gives the 2-D answer, 7 scipy's
    answer for the (1, Y, Z) array - nothing filled, every voxel lies on a border of the first axis."""
    rng = np.random.default_rng(65)
    seg = (rng.random((33, 65)) < 0.62).astype(np.uint8)
    seg[4:30, 40:60] = 1; seg[8:26, 44:56] = 0; seg[12, 50] = 2               # a ring across the 32 x 32 tiles, a label inside
    want = ref.fill_holes_ref(seg, [1])
    assert (want != seg).sum() > 50
    _check_holes(seg, labels_or_regions=[1])
    for conn in (6, 26):
        _check_small(seg, labels_or_regions=[1], min_size=5, connectivity=conn)
    table = np.array([-1, 0], np.int32)
    got, filled = _entry_holes(seg[None], table, 0, 1, 6)
    assert np.array_equal(got[0], want) and filled == (want != seg).sum()
    got, filled = _entry_holes(seg[None], table, 0, 1, 7)
    assert np.array_equal(got, ref.fill_holes_ref(seg[None], [1])) and np.array_equal(got, seg[None]) and filled == 0


def test_many_tiles_merge_on_smoothed_noise(noise96):
    seg = noise96
    assert len(np.unique(seg)) == 13
    labels = list(range(1, 13))
    sizes = [5 * k for k in labels]
    for conn in (6, 26):
        got = _check_small(seg, labels_or_regions=labels, min_size=sizes, connectivity=conn, per_member=True)
        assert (got != seg).any()
        _check_small(seg, labels_or_regions=labels, min_size=400, connectivity=conn)
    changed = 0
    for lab in (1, 6, 12):
        changed += int((_check_holes(seg, labels_or_regions=[lab]) != seg).sum())
    got = _check_holes(seg, labels_or_regions=[tuple(labels)], fill_label=12)
    assert changed + int((got != seg).sum()) > 0


# ---- values -----------------------------------------------------------------------------------------------------------
def test_uint16_maps_with_labels_above_255_and_another_background():
    seg = _blobs((19, 21, 37), 5, seed=16, dtype=np.uint16)
    seg[seg > 0] += 297                                                       # labels 298 .. 302, background 0
    seg[seg == 0] = 1000
    seg[4:12, 5:16, 9:31] = 299; seg[6:10, 7:14, 11:29] = 1000                  # a hollow box across the tile faces
    for conn in (6, 26):
        _check_small(seg, labels_or_regions=[298, (299, 300), 302], min_size=[4, 30, 9], connectivity=conn, per_member=True,
                     background_label=1000)
        _check_small(seg, labels_or_regions=[(298, 299, 300, 301, 302)], min_size=50, connectivity=conn, background_label=7)
    for lab in (299, 301):
        got = _check_holes(seg, labels_or_regions=[lab], background_label=1000)
        assert (got != seg).any() == (lab == 299)
    got = _check_holes(seg, labels_or_regions=[(298, 299, 300, 301, 302)], fill_label=65535, background_label=1000)
    assert (got == 65535).any()
    t = torch.from_numpy(seg.astype(np.int32)).to(DEV)                         # an int32 device tensor comes back as one
    out = _pp().fill_holes_in_segmentation(t, [(298, 299, 300, 301, 302)], fill_label=65535, background_label=1000)
    assert out.dtype == torch.int32 and out.device == t.device and np.array_equal(out.cpu().numpy(), got.astype(np.int32))


def test_labels_at_and_beyond_the_table_belong_to_no_set():
    """The entry with a table shorter than the map's values: value n_table and above are in no set (small components) and
    outside S (holes)."""
    rng = np.random.default_rng(4)
    seg = (rng.random((19, 21, 37)) < 0.3).astype(np.uint8) * rng.integers(1, 5, (19, 21, 37)).astype(np.uint8)   # values 0..4
    table = np.array([-1, 0, 1], np.int32)                                     # n_table 3: labels 3 and 4 lie beyond it
    got, removed = _entry_small(seg, table, 2, [5, 7], 26)
    want = ref.remove_small_ref(seg, [1, 2], [5, 7], per_member=True)
    assert np.array_equal(got, want) and np.array_equal(got[seg >= 3], seg[seg >= 3])
    assert removed.tolist() == [int(((seg == 1) & (want == 0)).sum()), int(((seg == 2) & (want == 0)).sum())]
    dense = np.where(rng.random((19, 21, 37)) < 0.75, rng.integers(1, 5, (19, 21, 37)), 0).astype(np.uint8)
    got, filled = _entry_holes(dense, np.array([-1, 0, 0], np.int32), 0, 2, 7)
    want = ref.fill_holes_ref(dense, [(1, 2)], fill_label=2)
    assert np.array_equal(got, want) and filled == (want != dense).sum()


def test_small_component_entry_counts_and_no_ops():
    seg = _blobs((19, 21, 37), 4, seed=2)
    table = np.array([-1, 0, 1, 2, 3], np.int32)
    for conn in (6, 26):
        sizes = [0, 1, 12, 10 ** 12]                                           # two no-ops, a filter, everything
        got, removed = _entry_small(seg, table, 4, sizes, conn, bg=0)
        want = ref.remove_small_ref(seg, [1, 2, 3, 4], sizes, connectivity=conn, per_member=True)
        assert np.array_equal(got, want)
        assert removed.tolist() == [0, 0, int(((seg == 3) & (want == 0)).sum()), int((seg == 4).sum())]
        assert np.array_equal(got[seg <= 2], seg[seg <= 2]) and not (got == 4).any()
        got, removed = _entry_small(seg, table, 4, [0, 1, -5, 1], conn)        # all no-ops: nothing is launched
        assert np.array_equal(got, seg) and removed.tolist() == [0, 0, 0, 0]


def test_small_component_entry_refuses_other_connectivities_on_a_device_map():
    from fast_nnunet_amd import capi
    t = torch.zeros((4, 4, 4), dtype=torch.uint8, device=DEV)
    with pytest.raises(NotImplementedError, match='connectivity must be 6 or 26'):        # FNN_E_UNSUPPORTED
        capi.remove_small_components(t.data_ptr(), False, t.shape, np.array([-1, 0], np.int32), 1, 0, [3], 18)


# ---- holes: the set and its box -----------------------------------------------------------------------------------------
def test_holes_with_an_empty_set_and_a_set_that_is_the_whole_volume():
    seg = np.full((19, 21, 37), 3, np.uint8)
    assert np.array_equal(_check_holes(seg, labels_or_regions=[1]), seg)                    # S empty
    assert np.array_equal(_check_holes(seg, labels_or_regions=[3], background_label=1), seg)   # S everything
    got, filled = _entry_holes(seg, np.array([-1, -1, -1, 0], np.int32), 0, 3, 7)
    assert np.array_equal(got, seg) and filled == 0
    seg[5:9, 5:9, 5:9] = 0                                                     # S is everything but a cavity
    got = _check_holes(seg, labels_or_regions=[3])
    assert (got == 3).all()
    seg[:] = 0; seg[5:9, 5:9, 5:9] = 3                                         # S fills its box: nothing inside to label
    got, filled = _entry_holes(seg, np.array([-1, -1, -1, 0], np.int32), 0, 3, 7)
    assert np.array_equal(got, seg) and filled == 0


def test_a_cavity_open_to_a_volume_face_that_the_box_touches_is_not_filled():
    """A cup whose rim lies on the face x = 0 of the volume: the cavity reaches that face.  The same cup one voxel inside the
    volume is open through its rim as well; closed with a lid, its cavity is filled."""
    for x0 in (0, 1):
        seg = np.zeros((12, 14, 40), np.uint8)
        seg[x0:x0 + 6, 3:11, 10:30] = 1
        seg[x0:x0 + 5, 4:10, 11:29] = 0                                         # hollow, open towards x = x0
        assert np.array_equal(_check_holes(seg, labels_or_regions=[1]), seg)
        if x0:
            seg[x0 - 1, 3:11, 10:30] = 1                                         # the lid; the box now touches x = 0
            got = _check_holes(seg, labels_or_regions=[1])
            assert (got != seg).sum() == 5 * 6 * 18
    seg = np.zeros((12, 14, 40), np.uint8)                                      # the box touches every face of the volume
    seg[0, :, :] = 1; seg[-1, :, :] = 1; seg[:, 0, :] = 1; seg[:, -1, :] = 1; seg[:, :, 0] = 1; seg[:, :, -1] = 1
    seg[3, 3, 3] = 4
    got = _check_holes(seg, labels_or_regions=[1])
    assert (got[1:-1, 1:-1, 1:-1] == 1).sum() == 10 * 12 * 38 - 1 and got[3, 3, 3] == 4
    seg[0, 5, 5] = 0                                                            # a hole in the wall that lies on the face
    assert np.array_equal(_check_holes(seg, labels_or_regions=[1]), seg)


def test_hole_entry_counts_and_region_with_explicit_fill():
    seg = _blobs((33, 5, 130), 3, seed=12, sigma=1.2, level=0.35)
    table = np.array([-1, 0, -1, 0], np.int32)                                 # S = {1, 3}
    got, filled = _entry_holes(seg, table, 0, 2, 7)
    want = ref.fill_holes_ref(seg, [(1, 3)], fill_label=2)
    assert np.array_equal(got, want) and filled == (want != seg).sum()
    big = _blobs((40, 40, 40), 2, seed=3, sigma=2.5, level=0.3)
    want = ref.fill_holes_ref(big, [(1, 2)], fill_label=1)
    got, filled = _entry_holes(big, np.array([-1, 0, 0], np.int32), 0, 1, 7)
    assert np.array_equal(got, want) and filled == (want != big).sum()


# ---- idempotence and determinism ------------------------------------------------------------------------------------------
def test_fill_holes_twice_equals_once_and_runs_repeat_bit_for_bit(noise96):
    pp = _pp()
    seg = noise96
    for kw in (dict(labels_or_regions=[3]), dict(labels_or_regions=[(1, 2, 3, 4)], fill_label=9)):
        once = pp.fill_holes_in_segmentation(seg, **kw)
        assert np.array_equal(pp.fill_holes_in_segmentation(once, **kw), once)
        assert once.tobytes() == pp.fill_holes_in_segmentation(seg, **kw).tobytes()
    kw = dict(labels_or_regions=list(range(1, 13)), min_size=60, connectivity=6, per_member=True)
    once = pp.remove_small_components_from_segmentation(seg, **kw)
    assert once.tobytes() == pp.remove_small_components_from_segmentation(seg, **kw).tobytes()
    assert np.array_equal(pp.remove_small_components_from_segmentation(once, **kw), once)


# ---- through the front ends ---------------------------------------------------------------------------------------------
def _shift_labels(segmentation, by):
    """A step of the caller's own (runs on the host): every foreground label moved up."""
    out = segmentation.copy()
    out[segmentation > 0] += by
    return out


def _mixed_steps(pp):
    fns = [pp.remove_all_but_largest_component_from_segmentation, pp.remove_small_components_from_segmentation,
           pp.remove_small_components_from_segmentation, pp.fill_holes_in_segmentation, pp.fill_holes_in_segmentation, _shift_labels,
           pp.remove_small_components_from_segmentation]
    kws = [{'labels_or_regions': [1, 2, 3, 4]}, {'labels_or_regions': 1, 'min_size': 30}, {'labels_or_regions': [2, 3], 'min_size': 20, 'connectivity': 26},
           {'labels_or_regions': 1}, {'labels_or_regions': [(2, 3)], 'fill_label': 3}, {'by': 1},
           {'labels_or_regions': [2, 3, 4, 5], 'min_size': 25, 'connectivity': 6, 'per_member': True}]
    kinds = ['largest', 'small', 'small', 'holes', 'holes', _shift_labels, 'small']
    return fns, kws, list(zip(kinds, kws))


def test_apply_postprocessing_of_a_mixed_list_equals_the_model_step_by_step():
    pp = _pp()
    seg = _blobs((40, 44, 48), 4, seed=21)
    seg[5:15, 5:15, 5:15] = 1; seg[7:13, 7:13, 7:13] = 0                       # two hollow boxes, a foreign label in one cavity
    seg[20:32, 20:32, 20:32] = 2; seg[23:29, 23:29, 23:29] = 0; seg[25, 25, 25] = 4
    fns, kws, steps = _mixed_steps(pp)
    assert [k for k, _ in pp.plan_passes(fns, kws)] == ['gpu', 'gpu_small', 'gpu_holes', 'gpu_holes', 'host', 'gpu_small']
    want = ref.apply_ref(seg, steps)
    assert (want != ref.apply_ref(seg, steps[:1])).any() and (ref.apply_ref(seg, steps[:3]) != ref.apply_ref(seg, steps[:5])).any()
    before = seg.copy()
    got = pp.apply_postprocessing(seg, fns, kws)
    assert np.array_equal(seg, before)
    _same(got, want, seg)
    t = torch.from_numpy(seg).to(DEV)
    out = pp.apply_postprocessing(t, fns, kws)
    assert out.device == t.device and np.array_equal(out.cpu().numpy(), want) and np.array_equal(t.cpu().numpy(), seg)


def test_predictor_with_the_new_steps_writes_what_the_folder_route_makes_of_the_plain_prediction(tmp_path):
    import nifti_ref
    from fast_nnunet_amd import nnUNetPredictor
    from test_gpu_predictor import _toy_model_folder
    pp = _pp()
    folder, plans, dj, sd, spec = _toy_model_folder(tmp_path, (16, 16, 32), 3, plans_spacing=(3.0, 3.0, 3.0))
    p = nnUNetPredictor(tile_step_size=0.5, use_gaussian=True, use_mirroring=False, device=DEV, allow_tqdm=False,
                        patches_per_forward=4)
    p.initialize_from_trained_model_folder(str(folder), use_folds=(0,))
    src = tmp_path / 'in'
    src.mkdir()
    for name, seed in (('a', 41), ('b', 42)):                                    # int16 noise with a zero border, 3 mm spacing
        v = (np.random.default_rng(seed).standard_normal((18, 20, 36)) * 300 + 100).astype(np.int16)
        v[:2] = 0
        v[:, :, -3:] = 0
        sform = np.diag([3.0, 3.0, 3.0, 1.0])
        sform[:3, 3] = [-10.0, 20.5, 3.0]
        nifti_ref.write(str(src / f'{name}_0000.nii.gz'), v, 4, sform=sform, sform_code=2, pixdim=(1, 3.0, 3.0, 3.0))
    p.predict_from_files(str(src), str(tmp_path / 'plain'))
    fns = [pp.remove_small_components_from_segmentation, pp.fill_holes_in_segmentation, pp.fill_holes_in_segmentation]
    kws = [{'labels_or_regions': [1, 2], 'min_size': 12, 'connectivity': 6, 'per_member': True}, {'labels_or_regions': 1}, {'labels_or_regions': 2}]
    p.set_postprocessing((fns, kws))
    try:
        p.predict_from_files(str(src), str(tmp_path / 'pp'))
    finally:
        p.set_postprocessing(None)
    pp.apply_postprocessing_to_folder(str(tmp_path / 'plain'), str(tmp_path / 'applied'), fns, kws, plans, dj)
    changed = 0
    for name in ('a', 'b'):
        plain = nifti_ref.read(str(tmp_path / 'plain' / f'{name}.nii.gz'))[0]
        got = nifti_ref.read(str(tmp_path / 'pp' / f'{name}.nii.gz'))[0]
        applied = nifti_ref.read(str(tmp_path / 'applied' / f'{name}.nii.gz'))[0]
        want = ref.apply_ref(plain, [('small', kws[0]), ('holes', kws[1]), ('holes', kws[2])])
        assert np.array_equal(got, applied) and np.array_equal(got, want)
        changed += int((got != plain).sum())
    assert changed > 0, 'the steps changed nothing: the case shows nothing'
