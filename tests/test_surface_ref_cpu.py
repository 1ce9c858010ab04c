"""The yardstick of the surface-distance tests (tests/surface_ref.py) against scipy, and the host half of the surface
metrics - no GPU.  scipy's binary_erosion and distance_transform_edt are what medpy's hd / hd95 / assd are made of."""
import numpy as np
import pytest

import surface_ref as sr

SPACINGS = {'unit': ((1.0, 1.0, 1.0), True), 'dyadic': ((2.0, 0.5, 0.25), True), 'ct': ((2.5, 0.7421875, 0.7421875), False)}


def _dilate(m):
    out = m.copy()
    for ax in range(3):
        lo, hi = [slice(None)] * 3, [slice(None)] * 3
        lo[ax], hi[ax] = slice(0, -1), slice(1, None)
        out[tuple(hi)] |= m[tuple(lo)]
        out[tuple(lo)] |= m[tuple(hi)]
    return out


def _masks(seed):
    rng = np.random.default_rng(seed)
    shape = tuple(int(n) for n in rng.integers(1, 24, 3))
    a = _dilate(rng.random(shape) < 0.05)
    b = _dilate(rng.random(shape) < 0.05) if seed % 3 else np.roll(a, 1, axis=int(np.argmax(shape)))
    return a, b


@pytest.mark.parametrize('name', sorted(SPACINGS))
def test_the_yardstick_equals_scipy(name):
    from scipy import ndimage as ndi
    spacing, exact = SPACINGS[name]
    structure = ndi.generate_binary_structure(3, 1)
    done = 0
    for seed in range(60):
        a, b = _masks(1000 + seed)
        sa, sb = sr.surface(a), sr.surface(b)
        for m, s in ((a, sa), (b, sb)):
            assert np.array_equal(s, m & ~ndi.binary_erosion(m, structure, border_value=0))
        if not (a.any() and b.any()):
            continue
        done += 1
        for (x, y, sx, sy) in ((a, b, sa, sb), (b, a, sb, sa)):
            want = ndi.distance_transform_edt(~sy, sampling=spacing)[sx]
            got = np.sqrt(sr.sq_distances(x, y, spacing))
            if exact:
                assert np.array_equal(got, want), (seed, np.flatnonzero(got != want)[:5])
            else:
                np.testing.assert_allclose(got, want, rtol=1e-12, atol=0)
    assert done >= 20


def test_case_lays_the_buffer_out_region_after_region():
    ref = np.zeros((4, 5, 6), np.uint8)
    pred = np.zeros((4, 5, 6), np.uint8)
    ref[1, 1, 1], pred[1, 1, 3] = 1, 1
    ref[2, 2, 2] = 2                                                    # only in ref
    ref[3, 4, 5], pred[0, 4, 5], pred[3, 4, 4] = 3, 3, 3
    n_surface, boxes, sq = sr.case(ref, pred, [1, 2, 3, (1, 3)], (2.0, 1.0, 0.5))
    assert n_surface.tolist() == [[1, 1], [1, 0], [1, 2], [2, 3]]
    assert boxes.tolist() == [[1, 2, 1, 2, 1, 4], [2, 3, 2, 3, 2, 3], [0, 4, 4, 5, 4, 6], [0, 4, 1, 5, 1, 6]]
    assert sq[:2].tolist() == [1.0, 1.0]                                # label 1: pred -> ref, ref -> pred
    assert sq[2:5].tolist() == [36.0, 0.25, 0.25]                       # label 3: its two pred voxels in raster order, then ref's
    assert len(sq) == 2 + 3 + 5


def test_metric_expressions_on_hand_made_distances():
    from fast_nnunet_amd import evaluation as ev
    dp, dr = np.array([0.0, 1.0, 2.0, 5.0]), np.array([1.0, 3.0])
    for fn in (sr.metrics, ev.surface_metrics_of):
        m = fn(dp, dr, 4, 2, 1.0)
        assert list(m) == ['HD', 'HD95', 'ASSD', 'NSD', 'n_surf_pred', 'n_surf_ref']
        assert m['HD'] == 5.0 and m['ASSD'] == 2.0 and m['NSD'] == 0.5 and m['n_surf_pred'] == 4 and m['n_surf_ref'] == 2
        assert m['HD95'] == np.percentile(np.array([0.0, 1.0, 2.0, 5.0, 1.0, 3.0]), 95) and 4.4 < m['HD95'] < 4.6
        assert fn(dp, dr, 4, 2, 0.5)['NSD'] == 1 / 6
    got, want = ev.surface_metrics_of(dp, dr, 4, 2, 2.0), sr.metrics(dp, dr, 4, 2, 2.0)
    assert all(got[k] == want[k] and type(got[k]) in (np.float64, np.int64) for k in sr.KEYS)


def test_an_empty_side_gives_nan():
    from fast_nnunet_amd import evaluation as ev
    for n_p, n_r in ((0, 3), (3, 0), (0, 0)):
        m = ev.surface_metrics_of(np.zeros(0), np.zeros(0), n_p, n_r, 1.0)
        assert all(np.isnan(m[k]) for k in ('HD', 'HD95', 'ASSD', 'NSD'))
        assert (m['n_surf_pred'], m['n_surf_ref']) == (n_p, n_r)
    empty, full = np.zeros((3, 3, 3), bool), np.ones((3, 3, 3), bool)
    assert np.isnan(sr.case_metrics(empty, full, [1], (1, 1, 1))[1]['HD'])


def test_surface_metrics_refuse_an_ignore_label_before_any_gpu_call():
    from fast_nnunet_amd import evaluation as ev
    seg = np.zeros((3, 4, 5), np.uint8)
    with pytest.raises(ValueError, match='surface metrics are refused together with an ignore label'):
        ev.compute_metrics(seg, seg, [1], ignore_label=2, surface_metrics=True, spacing=(1, 1, 1))
    with pytest.raises(ValueError, match='surface metrics are refused together with an ignore label'):
        ev.compute_metrics_on_arrays([seg], [seg], [1], ignore_label=2, surface_metrics=True, spacing=(1, 1, 1))
    with pytest.raises(ValueError, match='surface metrics are refused together with an ignore label'):
        ev.compute_metrics_on_files(['a.nii.gz'], ['b.nii.gz'], None, [1], ignore_label=2, surface_metrics=True)
    with pytest.raises(ValueError, match='need the voxel spacing'):
        ev.compute_metrics(seg, seg, [1], surface_metrics=True)


def test_region_members_and_tolerances():
    from fast_nnunet_amd import evaluation as ev
    assert ev.region_members([1, (2, 3), 5]).tolist() == [[0, 1, 0, 0, 0, 0], [0, 0, 1, 1, 0, 0], [0, 0, 0, 0, 0, 1]]
    with pytest.raises(ValueError, match='outside 0..65535'):
        ev.region_members([70000])
    with pytest.raises(ValueError, match='names no tolerance'):
        ev._tolerance_of({1: 2.0}, (1, 2))
    assert ev._tolerance_of({(1, 2): 2}, (1, 2)) == 2.0 and ev._tolerance_of(3, 1) == 3.0


def test_without_the_flag_a_case_has_exactly_the_eight_keys():
    from fast_nnunet_amd import evaluation as ev
    counts = np.array([[5, 1, 0], [2, 7, 0], [1, 0, 90]])
    metrics = ev.metrics_from_counts(counts, [1, 2])
    for r in (1, 2):
        assert list(metrics[r]) == ['Dice', 'IoU', 'FP', 'TP', 'FN', 'TN', 'n_pred', 'n_ref']
    summary = ev.aggregate([ev.case_result(metrics)], [1, 2])
    assert sorted(summary['mean'][1]) == sorted(['Dice', 'IoU', 'FP', 'TP', 'FN', 'TN', 'n_pred', 'n_ref'])
    with_surface = ev._with_surface(ev.metrics_from_counts(counts, [1, 2]),
                                    {r: ev.surface_metrics_of(np.array([1.0]), np.array([2.0]), 1, 1, 1.0) for r in (1, 2)})
    summary = ev.aggregate([ev.case_result(with_surface), ev.case_result(with_surface)], [1, 2])
    assert list(with_surface[1])[8:] == list(sr.KEYS) and summary['mean'][2]['HD'] == 2.0 and summary['foreground_mean']['ASSD'] == 1.5
