"""tests/prep_ref.py without a GPU: the references agree with the oracle, and EVERY case tests/test_gpu_prep_ops.py
commits discriminates - a reference with the mistake the case is meant to catch (26-connectivity, no fill, a grid-stride
loop that stops after one trip, a fused rounding, an unclipped resize) gives another answer than the reference."""
import os
import sys

import numpy as np
import pytest
from scipy import ndimage as ndi

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import prep_ref as R  # noqa: E402
from oracle import preprocess as opre  # noqa: E402
from oracle import resample as ores  # noqa: E402


# ---- the references against the oracle ----------------------------------------------------------------------------------
@pytest.mark.parametrize('tf', R.PERMS)
def test_bbox_and_mask_are_the_oracles(tf):
    raw = R.bbox_case('ragged')
    t = R.transpose_raw(raw, tf)
    assert R.bbox(raw, tf) == opre.nonzero_bbox(t)
    assert np.array_equal(R.filled_mask(t), opre.filled_nonzero_mask(t))
    assert np.array_equal(R.transpose_raw(R.to_raw(t, tf), tf), t)


def test_stats64_is_exact_where_float32_sums_are_not():
    x = np.full(1 << 20, 16384.0, np.float32)
    x[::2] += np.float32(0.001953125)
    mean, std = R.stats64(x)
    assert mean == 16384.0 + 0.001953125 / 2 and std == 0.001953125 / 2
    a, b = R.zscore_candidates(x)[4][0]
    assert a == np.float32(mean) and b == np.float32(std)


# ---- (a) box cases ------------------------------------------------------------------------------------------------------
def test_box_cases_are_what_their_names_say():
    full = [[0, n] for n in R.BBOX_SHAPE[1:]]
    tf = (0, 1, 2)
    assert R.bbox(R.bbox_case('all_zero'), tf) == full and R.bbox(R.bbox_case('negative_zero_only'), tf) == full
    assert np.signbit(R.bbox_case('negative_zero_only')).all()
    assert R.bbox(R.bbox_case('single_nan'), tf) == [[5, 6], [22, 23], [28, 29]]
    assert R.bbox(R.bbox_case('single_voxel'), tf) == [[16, 17], [0, 1], [13, 14]]
    ragged = R.bbox(R.bbox_case('ragged'), tf)
    assert all(lo > 0 or hi < n for (lo, hi), n in zip(ragged, R.BBOX_SHAPE[1:])) and ragged[1][0] == 0
    only1 = R.bbox_case('channel_1_only')
    assert not only1[0].any() and R.bbox(only1, tf) == [[2, 9], [20, 22], [3, 4]]
    inner = [[7, 10], [9, 13], [11, 16]]
    for ax in range(3):
        for end in ('lo', 'hi'):
            want = [list(b) for b in inner]
            want[ax][end == 'hi'] = 0 if end == 'lo' else R.BBOX_SHAPE[1 + ax]
            assert R.bbox(R.bbox_case(f'face_{ax}{end}'), tf) == want
    # a permutation moves the box with the axes
    assert R.bbox(R.bbox_case('single_nan'), (2, 0, 1)) == [[28, 29], [5, 6], [22, 23]]


def test_box_stride_case_is_decided_past_the_first_trip():
    raw = R.bbox_stride_case()
    assert raw.size > R.BBOX_STRIDE and not raw.ravel()[:R.BBOX_STRIDE].any()
    cut = raw.copy()
    cut.ravel()[R.BBOX_STRIDE:] = 0                               # a loop that stops after one trip sees an empty image
    assert R.bbox(raw, (0, 1, 2)) == [[129, 132], [5, 101], [7, 128]] != R.bbox(cut, (0, 1, 2))


# ---- (b) mask cases -----------------------------------------------------------------------------------------------------
def _thin_fill(nz):
    """The fill of a kernel that does not count the two faces of a thin axis: holes filled slice by slice."""
    ax = int(np.argmin(nz.shape))
    return np.stack([ndi.binary_fill_holes(s) for s in np.moveaxis(nz, ax, 0)], ax)


@pytest.mark.parametrize('case', R.PERCOLATION_CASES, ids=lambda c: f"{'x'.join(map(str, c['shape']))}-{c['zero']}")
def test_percolation_cases_have_holes_and_outside(case):
    raw_t = R.percolation_case(case)
    box = [[lo, lo + n] for n, (lo, hi) in zip(case['shape'], case['margins'])]
    assert R.bbox(R.to_raw(raw_t, case['tf']), case['tf']) == box
    crop = raw_t[(slice(None), *[slice(lo, hi) for lo, hi in box])]
    nz, filled = R.nonzero_any(crop), R.filled_mask(crop)
    assert abs((~nz).mean() - case['zero']) < 0.03
    assert np.signbit(crop[crop == 0]).any() and not np.signbit(crop[crop == 0]).all()
    assert np.array_equal(filled, R.filled_mask(raw_t)[tuple(slice(lo, hi) for lo, hi in box)])      # the box restriction is exact
    holes, outside = int((filled & ~nz).sum()), int((~filled).sum())
    print(case, 'holes', holes, 'outside', outside)
    if min(case['shape']) >= 30:                                  # the cubes: both kinds in bulk on either side of the threshold
        assert holes >= 500 and outside >= 500
    elif min(case['shape']) >= 3:                                 # one interior layer of 298 x 5
        assert holes >= 20 and outside >= 300
    else:                                                         # extent 1 or 2: every voxel lies on a face, nothing is enclosed
        assert holes == 0 and outside >= 300
        assert not np.array_equal(_thin_fill(nz), filled)
    if min(case['shape']) >= 3:
        assert not np.array_equal(nz, filled)                     # skipping the fill
    if case['channels'] == 2:                                     # the any-channel mask is not one channel's
        assert not np.array_equal(crop[0] != 0, nz) and not np.array_equal(crop[1] != 0, nz)


def test_percolation_cases_cover_what_they_should():
    cs = R.PERCOLATION_CASES
    for s in R.PERCOLATION_SHAPES:
        mine = [c for c in cs if c['shape'] == s]
        assert {c['zero'] for c in mine} == set(R.PERCOLATION_FRACTIONS)
        assert {c['channels'] for c in mine} == {1, 2} and len({c['tf'] for c in mine}) == 3 and len({c['margins'] for c in mine}) == 3
    assert any(lo == 0 for m in R.MARGINS[1:] for lo, hi in m) and any(lo > 0 for m in R.MARGINS[1:] for lo, hi in m)


def test_small_mask_cases_discriminate():
    box, _ = R.mask_case('diagonal_contact')
    nz = R.nonzero_any(box)
    six, all26 = R.filled_mask(box), ndi.binary_fill_holes(nz, structure=np.ones((3, 3, 3), bool))
    assert six[3:5, 3:5, 3:5].all() and not all26[3:5, 3:5, 3:5].any() and not np.array_equal(six, all26)
    assert not six[5, 5, 5:9].any() and not six[0:3, 5, 4].any()
    raw_t, _ = R.mask_case('face_background_only')
    b = R.bbox(raw_t, (0, 1, 2))
    crop = raw_t[(slice(None), *[slice(lo, hi) for lo, hi in b])]
    assert crop.shape == (1, 6, 5, 9) and crop[0, 1:-1, 1:-1, 1:-1].all() and (crop == 0).sum() > 30
    assert np.array_equal(R.filled_mask(crop), R.nonzero_any(crop))
    box, _ = R.mask_case('nan_wall')
    room = (slice(3, 6), slice(3, 6), slice(3, 7))
    assert R.filled_mask(box)[room].all() and not R.filled_mask(box)[4, 0:2, 5].any()
    assert not R.filled_mask(np.nan_to_num(box))[room].any()      # NaN taken for zero: the corridor reaches the room


@pytest.mark.parametrize('name', R.MASK_CASES)
def test_sweep_model_reproduces_scipy_on_the_small_cases(name):
    raw_t, _ = R.mask_case(name)
    b = R.bbox(raw_t, (0, 1, 2))
    crop = raw_t[(slice(None), *[slice(lo, hi) for lo, hi in b])]
    assert np.array_equal(R.sweep_model(R.nonzero_any(crop))[1], R.filled_mask(crop))


def test_serpentine_needs_more_iterations_than_the_old_bound():
    """The model needs R / 2 iterations (one free row and one gap per iteration) on shortened copies; by that law the
    committed R needs more than 2 x 4096.  The full R is not simulated."""
    for r in (41, 201, 801):
        box = R.serpentine(r)
        assert R.bbox(box, (0, 1, 2)) == [[0, 3], [0, r], [0, 5]]
        its, mask = R.sweep_model(R.nonzero_any(box))
        assert its == r // 2 and np.array_equal(mask, R.filled_mask(box))
        assert (~mask).sum() == (box == 0).sum() > 2 * r - 8       # the whole corridor is outside
    assert R.SERPENTINE_R // 2 > 2 * R.SWEEP_CAP and R.SERPENTINE_R / 4 > R.SWEEP_CAP
    full = R.serpentine(R.SERPENTINE_R)
    assert np.array_equal(R.filled_mask(full), R.nonzero_any(full))


# ---- (c) statistics and apply cases -------------------------------------------------------------------------------------
def test_stats_stride_case_is_decided_past_the_first_trip():
    raw_t, tf, schemes, _ = R.exact_case('stats_stride')
    assert tf == (0, 1, 2) and R.bbox(raw_t, tf) == [[0, n] for n in raw_t.shape[1:]]        # box index = raw index
    flat = raw_t.reshape(2, -1)
    assert flat.shape[1] > R.STATS_STRIDE
    for c in range(2):
        head, tail = flat[c, :R.STATS_STRIDE], flat[c, R.STATS_STRIDE:]
        assert tail.min() < head.min() and tail.max() > head.max()
        assert tail.astype(np.float64).sum() > 100 * head.astype(np.float64).sum()
        assert abs(R.stats64(head)[0] - R.stats64(flat[c])[0]) > 100
    want = opre.normalize_channel(raw_t[0], schemes[0], None)
    cut = opre.normalize_channel(raw_t[0].reshape(-1)[:R.STATS_STRIDE], schemes[0], None)
    assert not np.array_equal(want.reshape(-1)[:R.STATS_STRIDE], cut)


@pytest.mark.parametrize('name', R.EXACT_CASES)
def test_exact_cases_hold_what_they_claim(name):
    raw_t, tf, schemes, props = R.exact_case(name)
    assert raw_t.shape[0] == len(schemes) == len(props) <= 8
    crop = R.crop(R.to_raw(raw_t, tf), tf, R.bbox(R.to_raw(raw_t, tf), tf))
    for c, s in enumerate(schemes):
        want = opre.normalize_channel(crop[c], s, props[c])
        assert np.isfinite(want).all()
        if s == 'CTNormalization':
            lo, hi = np.float32(props[c]['percentile_00_5']), np.float32(props[c]['percentile_99_5'])
            assert (crop[c] == lo).any() and (crop[c] == hi).any() and (crop[c] < lo).any() and (crop[c] > hi).any()
        if s == 'RescaleTo01Normalization' and name == 'edges':
            # the statistics are the crop box's: the zero margins would move the minimum
            assert not np.array_equal(opre.normalize_channel(raw_t[c], s, None)[tuple(slice(lo, hi) for lo, hi in R.bbox(raw_t, (0, 1, 2)))], want)
    if name == 'std_zero':
        assert props[0]['std'] == 0 and np.ptp(crop[1]) == 0
        assert np.abs(opre.normalize_channel(crop[0], schemes[0], props[0])).max() > 1e9
    if name == 'eight_channels':
        assert len(schemes) == 8 and len(set(schemes)) == 4


@pytest.mark.parametrize('name', R.ZSCORE_EXACT_CASES)
@pytest.mark.parametrize('masked', [False, True])
def test_zscore_candidates_are_distinct_and_a_fused_rounding_is_none_of_them(name, masked):
    raw_t, tf = R.zscore_exact_case(name)
    crop = R.crop(R.to_raw(raw_t, tf), tf, R.bbox(R.to_raw(raw_t, tf), tf))
    mask = R.filled_mask(crop) if masked else None
    x = crop[0]
    mean, std = R.stats64(x if mask is None else x[mask])
    assert abs(mean) / std <= 1e3
    cands = R.zscore_candidates(x, mask)
    assert len(cands) == 9
    for i in range(9):
        for j in range(i):
            assert not np.array_equal(cands[i][1], cands[j][1])
    inside = np.ones(x.shape, bool) if mask is None else mask
    if name != 'stats_stride':
        assert masked == (not inside.all())
        if masked:
            assert all(np.array_equal(y[~inside], x[~inside]) for _, y in cands) and (x[inside] == 0).sum() >= 18
    a, b = cands[4][0]
    fused = x.copy()
    fused[inside] = ((x[inside].astype(np.float64) - np.float64(a)) / np.float64(b)).astype(np.float32)
    recip = x.copy()
    recip[inside] = (x[inside] - a) * (np.float32(1) / b)
    for mutant in (fused, recip):
        assert min((mutant != y).mean() for _, y in cands) >= 0.01


@pytest.mark.parametrize('mean,std', R.ILL_CASES)
def test_badly_conditioned_cases_are_badly_conditioned(mean, std):
    x = R.ill_case(mean, std)
    m64, s64 = R.stats64(x)
    assert abs(m64 - mean) <= 1e-2 * std + np.spacing(np.float32(mean)) and 0.5 * std < s64 < 2 * std and m64 / s64 > 1e4
    # what the statistics kernel computed before its second pass, against the bound the device test sets
    truth = R.zscore_truth64(x[0])
    ref32 = opre.normalize_channel(x[0], 'ZScoreNormalization', None)
    mo, so = R.zscore_old_formula(x)
    old = R.apply32(x[0], np.float32(mo), max(np.float32(so), np.float32(1e-8)))
    bound = 2 * np.abs(ref32 - truth).max() + np.spacing(np.float32(np.abs(truth).max()))
    print('old formula', np.abs(old - truth).max(), 'numpy fp32', np.abs(ref32 - truth).max(), 'std', so, 'exact', s64)
    new = R.zscore_candidates(x[0])[4][1]
    assert np.abs(new - truth).max() <= bound
    if (mean, std) == (16384.0, 0.002):
        assert np.abs(old - truth).max() > bound


@pytest.mark.parametrize('scheme', R.NONFINITE_SCHEMES)
def test_nonfinite_cases_hold_one_nonfinite_voxel(scheme):
    for value in (np.nan, np.inf):
        x = R.nonfinite_case(scheme, value)
        assert (~np.isfinite(x)).sum() == 1 and R.bbox(x, (0, 1, 2)) == [[0, 6], [0, 7], [0, 8]]


# ---- (e) resample cases -------------------------------------------------------------------------------------------------
def test_resample_edge_cases_have_axes_of_one_and_two():
    for shape, new_shape, order, axis in R.RESAMPLE_EDGE_CASES:
        assert min(shape[1:]) <= 2
        x = np.random.default_rng(1).standard_normal(shape).astype(np.float32)
        assert ores.resample_data(x, new_shape, axis=axis, order=order, do_separate_z=axis is not None).shape == (shape[0], *new_shape)
    assert {min(s[1:]) for s, _, _, _ in R.RESAMPLE_EDGE_CASES} == {1, 2}


def test_resample_stride_case_clips_to_values_of_the_tail():
    shape, new_shape, order, axis = R.RESAMPLE_STRIDE
    x = R.resample_stride_input()
    flat = x.reshape(-1)
    assert flat.size > R.MINMAX_STRIDE
    head = flat[:R.MINMAX_STRIDE]
    assert head.max() < 500 and head.min() > -500 and flat.max() == 1000 and flat.min() == -1000
    want = ores.resample_data(x, new_shape, axis=axis, order=order, do_separate_z=False)
    assert (want == 1000).sum() >= 100 and (want == -1000).sum() >= 100
    unclipped = ndi.zoom(x[0].astype(np.float64), [o / i for o, i in zip(new_shape, shape[1:])], order=3, mode='nearest', grid_mode=True)
    assert (unclipped > 1000.01).sum() >= 20 and (unclipped < -1000.01).sum() >= 20        # the clip acts
    cut = np.clip(unclipped, head.min(), head.max()).astype(np.float32)                        # the range of the first trip alone
    assert np.abs(cut - want[0]).max() > 400
