"""The whole-volume kernels of csrc/prep.hip (bbox, mask_init, mask_sweep, stats, apply, revert) and the edge shapes of
csrc/resample.hip, op by op through the C ABI against the plain references of tests/prep_ref.py and the oracle.  The box, the
filled mask, CT / RescaleTo01 / RGBTo01 / None and the label revert are compared exactly; ZScore must be one of the nine
outputs that an exactly rounded mean and std (or their fp32 neighbours) give.  tests/test_prep_ref_cpu.py proves that each
case committed here discriminates."""
import os
import re
import sys
import time

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import prep_ref as R  # noqa: E402
from oracle import preprocess as opre  # noqa: E402

pytestmark = pytest.mark.gpu


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _device_bbox(raw, tf):
    from fast_nnunet_amd import capi
    d = _dev(raw)
    return capi.nonzero_bbox(d.data_ptr(), raw.shape, tf)


def _preprocess(raw, tf, box, norms):
    from fast_nnunet_amd import capi
    d = _dev(raw)
    out = torch.empty((raw.shape[0], *[hi - lo for lo, hi in box]), dtype=torch.float32, device='cuda')
    capi.preprocess(d.data_ptr(), raw.shape, tf, box, norms, out.data_ptr())
    return out.cpu().numpy()


# ---- (a) box ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', R.BBOX_CASES)
def test_bbox_matches_the_reference_under_every_permutation(name):
    raw = R.bbox_case(name)
    for tf in R.PERMS:
        assert _device_bbox(raw, tf) == R.bbox(raw, tf), tf


def test_bbox_takes_a_second_trip_of_its_grid_stride_loop():
    raw = R.bbox_stride_case()
    for tf in R.THREE_PERMS:
        assert _device_bbox(raw, tf) == R.bbox(raw, tf), tf


# ---- (b) mask -----------------------------------------------------------------------------------------------------------
def _check_mask(raw_t, tf, schemes):
    """ZScore with use_mask leaves the zeros outside the filled mask as they are and moves the zeros inside it to
    -mean / std != 0: the mask is read from the zeros of the output, exactly."""
    raw = R.to_raw(raw_t, tf)
    box = R.bbox(raw, tf)
    assert _device_bbox(raw, tf) == box
    got = _preprocess(raw, tf, box, [R.norm_desc(s, use_mask=True) for s in schemes])
    crop = R.crop(raw, tf, box)
    outside = ~R.filled_mask(crop)
    for c, s in enumerate(schemes):
        if s != 'ZScoreNormalization':
            continue
        zero = crop[c] == 0
        assert zero.sum() > 0 and np.array_equal((got[c] == 0)[zero], outside[zero]), ((got[c] == 0)[zero] != outside[zero]).sum()
        assert np.array_equal(_bits(got[c][outside]), _bits(crop[c][outside]))       # -0.0 stays -0.0
    return outside


@pytest.mark.parametrize('case', R.PERCOLATION_CASES, ids=lambda c: f"{'x'.join(map(str, c['shape']))}-{c['zero']}")
def test_filled_mask_on_percolation_maps(case):
    _check_mask(R.percolation_case(case), case['tf'], ['ZScoreNormalization'] * case['channels'])


@pytest.mark.parametrize('name', R.MASK_CASES)
def test_filled_mask_on_small_cases(name):
    raw_t, schemes = R.mask_case(name)
    for tf in R.THREE_PERMS:
        _check_mask(raw_t, tf, schemes)


def test_filled_mask_of_a_serpentine_that_needs_more_than_4096_iterations():
    """A corridor that crosses a (3, R, 5) box R / 2 times, R / 4 > 4096: the mask must be scipy's, or the call must fail
    naming non-convergence - never a wrong mask.  On the MI355X the sweeps converge and the test takes 0.3 s; behind the
    bound of 4096 iterations they used to stop at, 569 of the corridor's 32837 voxels were still inside after 38 s."""
    raw_t = R.serpentine(R.SERPENTINE_R)
    t0 = time.perf_counter()
    try:
        outside = _check_mask(raw_t, (0, 1, 2), ['ZScoreNormalization'])
    except RuntimeError as e:
        assert re.search('converge', str(e)), e
        print(f'serpentine: refused after {time.perf_counter() - t0:.2f} s: {e}')
        return
    print(f'serpentine: converged, {time.perf_counter() - t0:.2f} s including the reference')
    assert outside.sum() == (raw_t == 0).sum()


# ---- (c) statistics and apply -------------------------------------------------------------------------------------------
def _oracle_channel(x, scheme, props):
    with np.errstate(all='ignore'):
        if scheme == 'RGBTo01Normalization':       # the oracle asserts 0 <= x <= 255 first, which a NaN fails; the division is the operation
            return x / np.float32(255.)
        return opre.normalize_channel(x, scheme, props)


@pytest.mark.parametrize('name', R.EXACT_CASES)
def test_ct_rescale_rgb_none_are_bit_exact(name):
    raw_t, tf, schemes, props = R.exact_case(name)
    raw = R.to_raw(raw_t, tf)
    box = R.bbox(raw, tf)
    assert _device_bbox(raw, tf) == box
    got = _preprocess(raw, tf, box, [R.norm_desc(s, p) for s, p in zip(schemes, props)])
    crop = R.crop(raw, tf, box)
    for c, s in enumerate(schemes):
        if s != 'ZScoreNormalization':              # (that channel of the stride case: test_zscore_is_one_of_the_nine_candidates)
            assert np.array_equal(_bits(got[c]), _bits(opre.normalize_channel(crop[c], s, props[c]))), (c, s)


def test_constant_zscore_channel_divides_zero_by_1e_8():
    """std = 0: every voxel equals the mean (sums of 7.5 are exact in fp32 and fp64), so the output is 0 / 1e-8 = 0."""
    raw = np.full((1, 9, 10, 11), 7.5, np.float32)
    box = R.bbox(raw, (0, 1, 2))
    got = _preprocess(raw, (0, 1, 2), box, [R.norm_desc('ZScoreNormalization')])
    assert np.array_equal(_bits(got[0]), _bits(opre.normalize_channel(raw[0], 'ZScoreNormalization', None))) and not got.any()


def test_nine_channels_are_refused():
    from fast_nnunet_amd import capi
    raw = np.ones((9, 4, 5, 6), np.float32)
    d = _dev(raw)
    out = torch.empty(raw.shape, dtype=torch.float32, device='cuda')
    with pytest.raises(AssertionError, match='channels'):
        capi.nonzero_bbox(d.data_ptr(), raw.shape, (0, 1, 2))
    with pytest.raises(AssertionError, match='channels'):
        capi.preprocess(d.data_ptr(), raw.shape, (0, 1, 2), [[0, 4], [0, 5], [0, 6]], [R.norm_desc('NoNormalization')] * 9, out.data_ptr())


@pytest.mark.parametrize('name', R.ZSCORE_EXACT_CASES)
@pytest.mark.parametrize('masked', [False, True])
def test_zscore_is_one_of_the_nine_candidates(name, masked):
    """fp64 statistics rounded to fp32 (the mean and the std each within one fp32 neighbour of the exactly rounded value),
    then an fp32 subtraction and an fp32 division: bit for bit one of nine arrays, and the same one on a second run."""
    raw_t, tf = R.zscore_exact_case(name)
    raw = R.to_raw(raw_t, tf)
    box = R.bbox(raw, tf)
    crop = R.crop(raw, tf, box)
    cands = R.zscore_candidates(crop[0], R.filled_mask(crop) if masked else None)
    hits = []
    for _ in range(2):
        got = _preprocess(raw, tf, box, [R.norm_desc('ZScoreNormalization', use_mask=masked)])
        hits.append([i for i, (_, y) in enumerate(cands) if np.array_equal(_bits(got[0]), _bits(y))])
    print('candidates matched', hits)
    assert len(hits[0]) == 1 and hits[1] == hits[0]


@pytest.mark.parametrize('mean,std', R.ILL_CASES)
def test_zscore_on_badly_conditioned_channels_is_as_close_as_the_float32_route(mean, std):
    """|mean| / std of 3e4, 1e6 and 8e6 on 1.21 M voxels: max|got - truth64| <= 2 max|ref32 - truth64| + 1 ulp of the output,
    truth64 = (x - mean64) / std64 in float64 and ref32 the oracle's numpy fp32 route on the same input (the factor 2 for the
    roundings of the mean and the std to fp32).  Both maxima are printed; on the MI355X, got / ref32:
    (3e4, 1) 5.95e-06 / 3.95e-03, (1e6, 1) 1.93e-03 / 6.92e-02, (16384, 0.002) 1.008e-02 / 1.033e-02 - and 7.57 for the last
    with the variance taken as E[x^2] - mean^2 in one pass."""
    x = R.ill_case(mean, std)
    truth = R.zscore_truth64(x[0])
    ref32 = opre.normalize_channel(x[0], 'ZScoreNormalization', None)
    got = _preprocess(x, (0, 1, 2), R.bbox(x, (0, 1, 2)), [R.norm_desc('ZScoreNormalization')])[0]
    err, ref_err = np.abs(got - truth).max(), np.abs(ref32 - truth).max()
    print(f'mean {mean} std {std}: max|got - truth64| = {err:.6g}, max|ref32 - truth64| = {ref_err:.6g}')
    assert err <= 2 * ref_err + np.spacing(np.float32(np.abs(truth).max()))


@pytest.mark.parametrize('value', [np.nan, np.inf], ids=['nan', 'inf'])
@pytest.mark.parametrize('scheme', R.NONFINITE_SCHEMES)
def test_one_nonfinite_voxel_gives_what_numpy_gives(scheme, value):
    """min / max propagate NaN (RescaleTo01 turns all-NaN), an inf makes ZScore's std NaN and max(NaN, 1e-8) is NaN."""
    x = R.nonfinite_case(scheme, value)
    props = R.CT_PROPS if scheme == 'CTNormalization' else None
    got = _preprocess(x, (0, 1, 2), R.bbox(x, (0, 1, 2)), [R.norm_desc(scheme, props)])
    want = _oracle_channel(x[0], scheme, props)
    assert np.array_equal(got[0], want, equal_nan=True), (got[0][:1, :1], want[:1, :1])
    if scheme == 'ZScoreNormalization':             # masked: the same statistics (no zero in the channel), the same all-NaN result
        gotm = _preprocess(x, (0, 1, 2), R.bbox(x, (0, 1, 2)), [R.norm_desc(scheme, use_mask=True)])
        assert np.isnan(gotm).all() and np.isnan(want).all()


# ---- (d) revert ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('u16', [False, True], ids=['u8', 'u16'])
@pytest.mark.parametrize('box', [[[2, 6], [0, 9], [3, 4]], [[6, 7], [8, 9], [0, 1]], [[0, 7], [0, 9], [0, 11]]], ids=['inner', '1x1x1', 'whole'])
def test_revert_labels_under_every_permutation(box, u16):
    from fast_nnunet_amd import capi
    before = (7, 9, 11)                                             # transposed shape before cropping
    rng = np.random.default_rng(5)
    seg = rng.integers(1, 60000 if u16 else 255, [hi - lo for lo, hi in box]).astype(np.uint16 if u16 else np.uint8)
    for tf in R.PERMS:
        tb = [int(i) for i in np.argsort(tf)]
        want = opre.revert_labels(seg, box, before, tb, 300 if u16 else 4)
        d = _dev(seg.view(np.int16) if u16 else seg)
        out = torch.full(want.shape, -1 if u16 else 255, dtype=torch.int16 if u16 else torch.uint8, device='cuda')
        capi.revert_labels(d.data_ptr(), u16, box, before, tb, out.data_ptr())
        got = out.cpu().numpy()
        got = got.view(np.uint16) if u16 else got
        assert got.dtype == want.dtype and np.array_equal(got, want), tf


# ---- (d') the crop-box map shared by revert_kernel and export_prob_kernel (fnn_device.h, crop_box_voxel) ---------------------
CROP_BEFORE, CROP_BOX = (5, 6, 7), [[1, 4], [2, 5], [1, 6]]          # three extents, none a multiple of 4; inside on all six faces


@pytest.mark.parametrize('tf', R.PERMS, ids=lambda t: ''.join(map(str, t)))
def test_crop_box_map_of_revert_and_export_under_every_permutation(tf):
    """Labels exactly opre.revert_labels; probabilities by the rule of test_gpu_preprocess (5e-7 of the oracle's softmax,
    labels equal where the oracle's top two differ by more than 1e-6) - and outside the box, where nothing is computed,
    exactly the background's 1 / the others' 0 and label 0, at exactly the oracle's voxels."""
    from fast_nnunet_amd import capi
    tb = [int(i) for i in np.argsort(tf)]
    cropped = [hi - lo for lo, hi in CROP_BOX]
    rng = np.random.default_rng(11)
    grid = [CROP_BEFORE[j] for j in tb]
    st = torch.cuda.current_stream().cuda_stream
    for u16 in (False, True):
        seg = rng.integers(1, 60000 if u16 else 255, cropped).astype(np.uint16 if u16 else np.uint8)
        want = opre.revert_labels(seg, CROP_BOX, CROP_BEFORE, tb, 300 if u16 else 4)
        out = torch.full(want.shape, -1 if u16 else 255, dtype=torch.int16 if u16 else torch.uint8, device='cuda')
        capi.revert_labels(_dev(seg.view(np.int16) if u16 else seg).data_ptr(), u16, CROP_BOX, CROP_BEFORE, tb, out.data_ptr())
        got = out.cpu().numpy()
        assert np.array_equal(got.view(np.uint16) if u16 else got, want), (tf, u16)
        assert (want != 0).sum() == seg.size                      # (every cropped voxel landed somewhere: no label is 0)
    H = 3
    logits = (rng.standard_normal((H, *cropped)) * 3).astype(np.float32)
    want_l, want_p = opre.export_with_probabilities(logits, CROP_BOX, CROP_BEFORE, tb, 4)
    inside = opre.revert_labels(np.ones(cropped, np.uint8), CROP_BOX, CROP_BEFORE, tb, 4).astype(bool)
    for half in (False, True):
        lg = _dev(logits.astype(np.float16) if half else logits)
        wl, wp = (opre.export_with_probabilities(logits.astype(np.float16), CROP_BOX, CROP_BEFORE, tb, 4) if half else (want_l, want_p))
        probs = torch.full((H, *grid), -1.0, dtype=torch.float32, device='cuda')
        labels = torch.full(grid, 255, dtype=torch.uint8, device='cuda')
        capi.export_probabilities(lg.data_ptr(), half, H, None, CROP_BOX, CROP_BEFORE, tb, probs.data_ptr(), labels.data_ptr(), False, st)
        got_p, got_l = probs.cpu().numpy(), labels.cpu().numpy()
        assert np.array_equal(_bits(got_p[:, ~inside]), _bits(wp[:, ~inside])) and not got_l[~inside].any(), (tf, half)
        assert np.abs(got_p - wp).max() <= 5e-7, (tf, half)
        top2 = np.sort(wp, 0)[-2:]
        decided = (top2[1] - top2[0] > 1e-6) | (top2[1] == top2[0])
        assert decided.mean() > 0.99 and np.array_equal(got_l[decided], wl[decided]), (tf, half)


def test_crop_boxes_outside_their_grid_are_refused_in_both_wordings():
    """Behind the device-pointer check, so only a GPU reaches them: fnn_preprocess checks the box against the transposed
    image, fnn_revert_labels and fnn_export_probabilities against shape_before_cropping; an unknown normalisation scheme
    is refused before anything runs and writes nothing."""
    from fast_nnunet_amd import capi
    lib = capi.load_library()
    raw = _dev(np.ones((1, 4, 5, 6), np.float32))
    for box in ([[0, 7], [0, 5], [0, 4]], [[-1, 6], [0, 5], [0, 4]], [[0, 6], [2, 2], [0, 4]]):      # transposed (2, 1, 0): 6 x 5 x 4
        out = torch.empty(1, 6, 5, 4, device='cuda')
        with pytest.raises(AssertionError, match=re.escape('bbox outside the (transposed) image')):
            capi.preprocess(raw.data_ptr(), (1, 4, 5, 6), (2, 1, 0), box, [R.norm_desc('RGBTo01Normalization')], out.data_ptr())
    seg = torch.ones(4, 5, 6, dtype=torch.uint8, device='cuda')
    out = torch.empty(4, 5, 6, dtype=torch.uint8, device='cuda')
    with pytest.raises(AssertionError, match='bbox outside shape_before_cropping'):
        capi.revert_labels(seg.data_ptr(), False, [[0, 4], [0, 6], [0, 6]], (4, 5, 6), (0, 1, 2), out.data_ptr())
    import ctypes as C
    out = torch.full((1, 4, 5, 6), 7.0, device='cuda')
    desc = (capi.NormDesc * 1)(capi.NormDesc(77, 0.0, 1.0, 0.0, 1.0, 0))
    rc = lib.fnn_preprocess(raw.data_ptr(), (C.c_int64 * 4)(1, 4, 5, 6), (C.c_int32 * 3)(0, 1, 2), (C.c_int64 * 6)(0, 4, 0, 5, 0, 6),
                            desc, out.data_ptr(), None)
    assert rc == capi.FNN_E_UNSUPPORTED and lib.fnn_last_error(None) == b'unknown normalisation scheme'
    assert bool((out == 7.0).all())


# ---- (e) resample edges -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape,new_shape,order,axis', R.RESAMPLE_EDGE_CASES)
def test_resample_with_axes_of_length_one_and_two(shape, new_shape, order, axis):
    from test_gpu_preprocess import _resample_case
    _resample_case(shape, new_shape, order, axis)


def test_resample_clip_range_takes_a_second_trip_of_the_minmax_loop():
    """The tolerances of test_gpu_preprocess._resample_case on an input whose minimum and maximum lie past 2048 x 256."""
    from fast_nnunet_amd import capi
    from oracle import resample as ores
    shape, new_shape, order, axis = R.RESAMPLE_STRIDE
    x = R.resample_stride_input()
    want = ores.resample_data(x, new_shape, axis=axis, order=order, do_separate_z=False)
    out = torch.empty((shape[0], *new_shape), dtype=torch.float32, device='cuda')
    d = _dev(x)
    capi.resample(d.data_ptr(), shape, new_shape, order, axis, False, out.data_ptr())
    got = out.cpu().numpy()
    assert np.abs(got - want).max() <= 4 * 6e-8 * np.abs(want).max(), np.abs(got - want).max()
    assert (got == 1000).sum() >= 100 and (got == -1000).sum() >= 100
    xh = x.astype(np.float16)
    wanth = ores.resample_data(xh, new_shape, axis=axis, order=order, do_separate_z=False)
    outh = torch.empty((shape[0], *new_shape), dtype=torch.half, device='cuda')
    dh = _dev(xh)
    capi.resample(dh.data_ptr(), shape, new_shape, order, axis, True, outh.data_ptr())
    goth = outh.cpu().numpy()
    ulp = np.spacing(np.abs(wanth).astype(np.float16)).astype(np.float32)
    assert (np.abs(goth.astype(np.float32) - wanth.astype(np.float32)) <= ulp).all()
    assert (goth != wanth).mean() < 5e-3
