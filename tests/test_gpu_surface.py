"""fnn_surface_count / fnn_surface_distances and the boundary metrics on one MI355X against tests/surface_ref.py: surface
sizes, boxes and the whole buffer of squared distances equal elementwise and in order.

The kernels' line tiles: the y pass stages 128 elements of a line in LDS, the x pass 1024 raster-consecutive box voxels; the
z pass has none.  The shapes with one axis of 1030 cross each of them."""
import json
import os

import numpy as np
import pytest
import torch

import surface_ref as sr

pytestmark = pytest.mark.gpu

EXACT_SPACINGS = [(1.0, 1.0, 1.0), (2.0, 0.5, 0.25)]
CLOSE_SPACING = (2.5, 0.7421875, 0.7421875)
SHAPES = [(5, 7, 9), (17, 33, 70), (1, 40, 40), (40, 1, 1), (1, 1, 1), (1030, 3, 4), (3, 1030, 4), (3, 4, 1030)]
GUARD, SENTINEL = 8, -7.0


# ---- label maps
def dilate(m):
    out = m.copy()
    for ax in range(3):
        lo, hi = [slice(None)] * 3, [slice(None)] * 3
        lo[ax], hi[ax] = slice(0, -1), slice(1, None)
        out[tuple(hi)] |= m[tuple(lo)]
        out[tuple(lo)] |= m[tuple(hi)]
    return out


def blobs(shape, rng, n_labels=3, seeds=25):
    """``seeds`` voxels per label (at most one voxel in 20), dilated twice: the yardstick is quadratic in the surfaces."""
    seg = np.zeros(shape, np.uint8)
    for label in range(1, n_labels + 1):
        seg[dilate(dilate(rng.random(shape) < min(0.05, seeds / np.prod(shape))))] = label
    return seg


def perturbed(seg, rng, hi=3):
    pred = seg.copy()
    where = dilate(rng.random(seg.shape) < min(0.01, 60 / seg.size))
    pred[where] = rng.integers(0, hi + 1, seg.shape)[where]
    return pred


def shifted(seg, axis):
    out = np.zeros_like(seg)
    lo, hi = [slice(None)] * 3, [slice(None)] * 3
    lo[axis], hi[axis] = slice(0, -1), slice(1, None)
    out[tuple(hi)] = seg[tuple(lo)]
    return out


def s_blobs(shape, rng):
    ref = blobs(shape, rng)
    return ref, perturbed(ref, rng), [1, 2, 3]


def s_single(shape, rng):
    ref, pred = np.zeros(shape, np.uint8), np.zeros(shape, np.uint8)
    ref[tuple(int(rng.integers(0, n)) for n in shape)] = 1
    pred[tuple(int(rng.integers(0, n)) for n in shape)] = 1
    return ref, pred, [1]


def s_full(shape, rng):
    ref = np.ones(shape, np.uint8)
    pred = ref.copy()
    pred[tuple(slice(0, max(1, n // 2)) for n in shape)] = 0
    return ref, pred, [1]


def s_faces(shape, rng):
    ref = np.ones(shape, np.uint8)
    ref[tuple(slice(1, -1) for _ in shape)] = 0                         # a shell on every face
    ref[tuple(n // 2 for n in shape)] = 1
    pred = np.zeros(shape, np.uint8)
    mid = [n // 2 for n in shape]
    for ax in range(3):
        for end in (0, shape[ax] - 1):
            at = list(mid)
            at[ax] = end
            pred[tuple(at)] = 1                                         # one voxel on each face
    return ref, pred, [1]


def s_corners(shape, rng):
    ref, pred = np.zeros(shape, np.uint8), np.zeros(shape, np.uint8)
    ref[:2, :2, :2] = 1
    pred[-2:, -2:, -2:] = 1
    return ref, pred, [1]


def s_same(shape, rng):
    ref = blobs(shape, rng, seeds=40)
    return ref, ref.copy(), [1, 2, 3]


def s_checker(shape, rng):
    z, y, x = np.indices(shape)
    ref = ((z + y + x) % 2 == 0).astype(np.uint8)
    return ref, (1 - ref).astype(np.uint8), [1]


def s_shift(shape, rng):
    ref = blobs(shape, rng, seeds=30)
    return ref, shifted(ref, int(np.argmax(shape))), [1, 2, 3]


def s_presence(shape, rng):
    """Label 1 only in ref, 2 only in pred, 3 in neither, 4 and 5 in both; 200 is above the table; an empty region in
    the middle of the call."""
    ref = blobs(shape, rng, n_labels=5, seeds=20)
    pred = perturbed(ref, rng, hi=5)
    ref[ref == 2] = 0
    pred[pred == 1] = 0
    ref[ref == 3], pred[pred == 3] = 0, 0
    ref[rng.random(shape) < 0.02] = 200
    pred[rng.random(shape) < 0.02] = 200
    return ref, pred, [4, 1, 3, 2, 5, (4, 5), (1, 2, 3)]


def s_touching(shape, rng):
    """A region of two labels whose parts touch: the boundary between them is inside the region, not on its surface."""
    ref = np.zeros(shape, np.uint8)
    half = [max(1, n // 2) for n in shape]
    ref[:, :, :half[2]] = 1
    ref[:, :, half[2]:] = 2
    ref[:, :half[1]][ref[:, :half[1]] == 2] = 1
    ref[-1:, -1:, -1:] = 0
    pred = shifted(ref, int(np.argmax(shape)))
    return ref, pred, [(1, 2), 1, 2]


SCENARIOS = {'blobs': s_blobs, 'single': s_single, 'full': s_full, 'faces': s_faces, 'corners': s_corners, 'same': s_same,
             'checker': s_checker, 'shift': s_shift, 'presence': s_presence, 'touching': s_touching}
# the brute-force yardstick is quadratic in the surfaces: the dense masks stay off the largest shape, and on the long shapes
# they are cut to the last WINDOW voxels of the long axis, which cross a tile boundary of the y pass (896, 1024) and the one
# of the x pass (1024)
DENSE, WINDOW = ('full', 'checker', 'touching'), 150
CASES = [(name, shape) for shape in SHAPES for name in SCENARIOS if not (name in DENSE and shape == (17, 33, 70))]


def make(name, shape, wide=False):
    rng = np.random.default_rng(sum(shape) * 131 + sorted(SCENARIOS).index(name) * 7 + shape[0])
    ref, pred, regions = SCENARIOS[name](shape, rng)
    if name in DENSE and max(shape) > 1000:
        cut = [slice(None)] * 3
        cut[int(np.argmax(shape))] = slice(0, max(shape) - WINDOW)
        ref[tuple(cut)], pred[tuple(cut)] = 0, 0
    if wide:
        ref, pred = ref.astype(np.uint16), pred.astype(np.uint16)
    return ref, pred, regions


# ---- the two entries with guard words around the buffer
def run(ref, pred, regions, spacing, cap_short=0):
    from fast_nnunet_amd import capi, evaluation as ev
    u16 = ref.dtype != np.uint8 or pred.dtype != np.uint8
    dev = torch.device('cuda', 0)
    r, p = ev.to_device_labels(ref, u16, dev), ev.to_device_labels(pred, u16, dev)
    member = ev.region_members(regions)
    n_surface, boxes = capi.surface_count(r.data_ptr(), p.data_ptr(), u16, ref.shape, member)
    both = (n_surface[:, 0] > 0) & (n_surface[:, 1] > 0)
    total = int(n_surface[both].sum())
    buf = torch.full((total + 2 * GUARD,), SENTINEL, dtype=torch.float64, device=dev)
    try:
        capi.surface_distances(r.data_ptr(), p.data_ptr(), u16, ref.shape, member, spacing, buf.data_ptr() + 8 * GUARD,
                               total - cap_short)
    finally:
        out = buf.cpu().numpy()
        assert np.all(out[:GUARD] == SENTINEL) and np.all(out[GUARD + total:] == SENTINEL), 'guard words overwritten'
        if cap_short:
            assert np.all(out == SENTINEL), 'a refused call wrote distances'
    return n_surface, boxes, out[GUARD:GUARD + total]


def check(ref, pred, regions):
    for spacing in EXACT_SPACINGS + [CLOSE_SPACING]:
        want_n, want_box, want_sq = sr.case(ref, pred, regions, spacing)
        n_surface, boxes, sq = run(ref, pred, regions, spacing)
        assert np.array_equal(n_surface, want_n), (n_surface, want_n)
        assert np.array_equal(boxes, want_box), (boxes, want_box)
        assert sq.shape == want_sq.shape
        if spacing == CLOSE_SPACING:
            np.testing.assert_allclose(sq, want_sq, rtol=1e-12, atol=0)
        else:
            assert np.array_equal(sq, want_sq), (spacing, np.flatnonzero(sq != want_sq)[:5], sq[sq != want_sq][:5],
                                                 want_sq[sq != want_sq][:5])


@pytest.mark.parametrize('name,shape', CASES, ids=[f'{n}-{"x".join(map(str, s))}' for n, s in CASES])
def test_counts_boxes_and_distances_equal_the_yardstick(name, shape):
    ref, pred, regions = make(name, shape, wide=(len(name) + shape[2]) % 2 == 1)
    check(ref, pred, regions)


def test_uint16_maps_with_labels_above_255_and_a_region_the_uint8_maps_cannot_hold():
    ref, pred, _ = make('blobs', (17, 33, 70))
    wide_ref, wide_pred = ref.astype(np.uint16), pred.astype(np.uint16)
    wide_ref[ref == 2], wide_pred[pred == 2] = 300, 300
    wide_ref[0, 0, 0] = 65535
    check(wide_ref, wide_pred, [1, 300, (3, 300), 65535])
    check(ref, pred, [1, 300, (3, 300)])                                # uint8 maps: 300 belongs to nothing they hold


def test_a_mixed_pair_of_uint8_and_uint16_maps():
    ref, pred, regions = make('blobs', (5, 7, 9))
    check(ref, pred.astype(np.uint16), regions)


def test_more_than_64_regions():
    rng = np.random.default_rng(7)
    ref = rng.integers(0, 71, (6, 12, 14)).astype(np.uint8)
    ref = np.repeat(np.repeat(ref, 2, axis=1), 2, axis=2)
    pred = perturbed(ref, rng, hi=70)
    check(ref, pred, list(range(1, 71)) + [(3, 66, 70)])


def test_two_calls_give_identical_buffers():
    ref, pred, regions = make('presence', (17, 33, 70))
    a = run(ref, pred, regions, EXACT_SPACINGS[1])
    b = run(ref, pred, regions, EXACT_SPACINGS[1])
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()


def test_a_cap_one_short_is_refused_and_writes_nothing():
    from fast_nnunet_amd import capi
    ref, pred, regions = make('blobs', (17, 33, 70))
    with pytest.raises(AssertionError, match='fnn_surface_distances: cap is below the number of distances'):
        run(ref, pred, regions, EXACT_SPACINGS[0], cap_short=1)
    assert capi.load_library().fnn_last_error(None).decode().startswith('fnn_surface_distances: cap is below')


def test_an_empty_volume_gives_zeros():
    ref = np.zeros((0, 4, 5), np.uint8)
    n_surface, boxes, sq = run(ref, ref, [1, 2], EXACT_SPACINGS[0])
    assert not n_surface.any() and not boxes.any() and sq.size == 0


# ---- the Python functions
def same_value(a, b):
    return (isinstance(a, float) or isinstance(a, np.floating)) and np.isnan(a) and np.isnan(b) or a == b


@pytest.mark.parametrize('spacing', EXACT_SPACINGS)
def test_compute_surface_metrics_equals_the_yardstick(spacing):
    from fast_nnunet_amd import evaluation as ev
    ref, pred, regions = make('presence', (17, 33, 70))
    tol = {r: 0.5 + k for k, r in enumerate(regions)}
    got = ev.compute_surface_metrics(ref, pred, regions, spacing, tol)
    assert list(got) == regions
    for r in regions:
        want = sr.metrics(*_directed(ref, pred, r, spacing), tol[r])
        assert list(got[r]) == list(sr.KEYS)
        for k in sr.KEYS:
            assert same_value(got[r][k], want[k]), (r, k, got[r][k], want[k])
    assert np.isnan(got[1]['HD']) and np.isnan(got[3]['NSD']) and got[1]['n_surf_ref'] > 0 and got[1]['n_surf_pred'] == 0
    assert not np.isnan(got[4]['HD95'])
    dist = ev.surface_distances(torch.from_numpy(ref).cuda(), torch.from_numpy(pred), regions, spacing)
    for r in regions:
        dp, dr, _, _ = _directed(ref, pred, r, spacing)
        assert np.array_equal(dist[r][0], dp) and np.array_equal(dist[r][1], dr) and dist[r][0].dtype == np.float64


def _directed(ref, pred, r, spacing):
    mr, mp = sr.region_mask(ref, r), sr.region_mask(pred, r)
    n_r, n_p = int(sr.surface(mr).sum()), int(sr.surface(mp).sum())
    if not (n_r and n_p):
        return np.zeros(0), np.zeros(0), n_p, n_r
    return np.sqrt(sr.sq_distances(mp, mr, spacing)), np.sqrt(sr.sq_distances(mr, mp, spacing)), n_p, n_r


def test_compute_metrics_appends_the_six_keys_only_when_asked():
    from fast_nnunet_amd import evaluation as ev
    ref, pred, regions = make('blobs', (5, 7, 9))
    ref4, pred4 = ref[None], pred[None]                                 # the reference's [1, X, Y, Z]
    off = ev.compute_metrics(ref4, pred4, regions)['metrics']
    on = ev.compute_metrics(ref4, pred4, regions, surface_metrics=True, spacing=EXACT_SPACINGS[1], nsd_tolerance=0.5)['metrics']
    want = sr.case_metrics(ref, pred, regions, EXACT_SPACINGS[1], 0.5)
    for r in regions:
        assert list(off[r]) == ['Dice', 'IoU', 'FP', 'TP', 'FN', 'TN', 'n_pred', 'n_ref']
        assert list(on[r]) == list(off[r]) + list(sr.KEYS)
        assert all(same_value(on[r][k], off[r][k]) for k in off[r])
        assert all(same_value(on[r][k], want[r][k]) for k in sr.KEYS)
    summary = ev.compute_metrics_on_arrays([ref, ref], [pred, ref], regions, surface_metrics=True,
                                           spacing=[EXACT_SPACINGS[1], EXACT_SPACINGS[0]], nsd_tolerance=0.5)
    assert all(same_value(summary['metric_per_case'][0]['metrics'][r][k], float(want[r][k])) for r in regions for k in sr.KEYS)
    with pytest.raises(ValueError, match='spacing'):
        ev.compute_metrics(ref, pred, regions, surface_metrics=True)


# ---- folders
AFFINE = np.array([[-1.5, 0, 0, 10.0], [0, 2.0, 0, -20.5], [0, 0, 0.5, 3.0], [0, 0, 0, 1.0]])     # spacing (z, y, x) = (0.5, 2, 1.5)
SWAPPED = np.array([[0, 2.0, 0, 1.0], [-1.5, 0, 0, 2.0], [0, 0, 0.5, 3.0], [0, 0, 0, 1.0]])       # array x lies along world y
FOLDER_SHAPE = (9, 20, 31)
LABELS = [1, 2, 3]


def _folder_maps():
    rng = np.random.default_rng(99)
    refs = [blobs(FOLDER_SHAPE, rng, seeds=20) for _ in range(3)]
    preds = [perturbed(r, rng) for r in refs]
    refs[1][0, 0, 0] = 2
    preds[1][preds[1] == 2] = 0                                         # a label missing in the prediction
    return refs, preds


def _write(rw, folder, maps, affine):
    os.makedirs(folder, exist_ok=True)
    files = []
    for i, m in enumerate(maps):
        files.append(os.path.join(folder, f'case_{i}.nii.gz'))
        rw.write_seg(m, files[-1], {'nibabel_stuff': {'original_affine': affine}})
    return files


def _summary_checks(summary_file, off_file, wants):
    from fast_nnunet_amd import evaluation as ev
    got, off = ev.load_summary_json(summary_file), ev.load_summary_json(off_file)
    assert len(got['metric_per_case']) == len(wants)
    for case, case_off, want in zip(got['metric_per_case'], off['metric_per_case'], wants):
        for r in LABELS:
            assert list(case_off['metrics'][r]) == sorted(['Dice', 'IoU', 'FP', 'TP', 'FN', 'TN', 'n_pred', 'n_ref'])
            assert all(same_value(case['metrics'][r][k], v) for k, v in case_off['metrics'][r].items())
            for k in sr.KEYS:
                assert same_value(case['metrics'][r][k], float(want[r][k])), (r, k, case['metrics'][r][k], want[r][k])
    for r in LABELS:
        for k in sr.KEYS:
            vals = [float(w[r][k]) for w in wants]
            mean = np.nan if all(np.isnan(v) for v in vals) else float(np.nanmean(vals))
            assert same_value(got['mean'][r][k], mean), (r, k)
        assert all(same_value(got['mean'][r][k], v) for k, v in off['mean'][r].items())
    with open(summary_file) as f:
        assert 'HD95' in json.load(f)['foreground_mean']


def test_folder_summary_carries_the_surface_metrics(tmp_path):
    from fast_nnunet_amd import evaluation as ev
    from fast_nnunet_amd.imageio import NiftiIO
    refs, preds = _folder_maps()
    fr, fp = os.path.join(tmp_path, 'ref'), os.path.join(tmp_path, 'pred')
    _write(NiftiIO(), fr, refs, AFFINE), _write(NiftiIO(), fp, preds, AFFINE)
    on, off = os.path.join(tmp_path, 'on.json'), os.path.join(tmp_path, 'off.json')
    ev.compute_metrics_on_folder_simple(fr, fp, LABELS, on, surface_metrics=True, nsd_tolerance=1.5)
    ev.compute_metrics_on_folder_simple(fr, fp, LABELS, off)
    wants = [sr.case_metrics(r, p, LABELS, (0.5, 2.0, 1.5), 1.5) for r, p in zip(refs, preds)]
    assert np.isnan(wants[1][2]['HD']) and not np.isnan(wants[0][2]['HD'])
    _summary_checks(on, off, wants)


def test_a_pair_of_different_spacings_names_both_files(tmp_path):
    from fast_nnunet_amd import evaluation as ev
    from fast_nnunet_amd.imageio import NiftiIO
    refs, preds = _folder_maps()
    fr, fp = os.path.join(tmp_path, 'ref'), os.path.join(tmp_path, 'pred')
    other = AFFINE.copy()
    other[1, 1] = 2.5
    r, p = _write(NiftiIO(), fr, refs[:1], AFFINE), _write(NiftiIO(), fp, preds[:1], other)
    with pytest.raises(ValueError, match='spacing mismatch') as e:
        ev.compute_metrics_on_folder(fr, fp, None, NiftiIO(), '.nii.gz', LABELS, surface_metrics=True)
    assert r[0] in str(e.value) and p[0] in str(e.value)
    ev.compute_metrics_on_folder(fr, fp, None, NiftiIO(), '.nii.gz', LABELS)        # without the flag the pair is evaluated
    given = ev.compute_metrics_on_folder(fr, fp, None, NiftiIO(), '.nii.gz', LABELS, surface_metrics=True, spacing=(1.0, 1.0, 1.0))
    want = sr.case_metrics(refs[0], preds[0], LABELS, (1.0, 1.0, 1.0))                # a given spacing replaces the files'
    assert all(same_value(given['metric_per_case'][0]['metrics'][r_][k], float(want[r_][k])) for r_ in LABELS for k in sr.KEYS)


def test_a_reoriented_file_is_measured_with_the_reoriented_spacing(tmp_path):
    from fast_nnunet_amd import evaluation as ev
    from fast_nnunet_amd.imageio import NiftiIO, NiftiReorientIO
    refs, preds = _folder_maps()
    fr, fp = os.path.join(tmp_path, 'ref'), os.path.join(tmp_path, 'pred')
    r, p = _write(NiftiIO(), fr, refs[:1], SWAPPED), _write(NiftiIO(), fp, preds[:1], SWAPPED)
    rw = NiftiReorientIO()
    ref_ras, props = rw.read_label_map(r[0], on_device=False)
    pred_ras, _ = rw.read_label_map(p[0], on_device=False)
    _, file_props = NiftiIO().read_label_map(r[0], on_device=False)
    assert ref_ras.shape != refs[0].shape and list(props['spacing']) != list(file_props['spacing'])
    got = ev.compute_metrics_on_folder(fr, fp, None, rw, '.nii.gz', LABELS, surface_metrics=True, nsd_tolerance=1.5)
    want = sr.case_metrics(ref_ras, pred_ras, LABELS, props['spacing'], 1.5)
    wrong = sr.case_metrics(ref_ras, pred_ras, LABELS, file_props['spacing'], 1.5)
    assert any(not same_value(want[r_][k], wrong[r_][k]) for r_ in LABELS for k in sr.KEYS)
    for r_ in LABELS:
        for k in sr.KEYS:
            assert same_value(got['metric_per_case'][0]['metrics'][r_][k], float(want[r_][k])), (r_, k)
