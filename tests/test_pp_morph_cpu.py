"""Small-component removal and hole filling without a GPU: the scipy restatement (tests/pp_morph_ref.py) on hand-made maps
whose answer is written out, the pass planner on mixed lists, the pkl loader, and every refusal that comes from the
arguments alone - in Python (ValueError naming the argument) and in the C entries (code and text)."""
import ctypes as C
import os
import pickle

import numpy as np
import pytest

import pp_morph_ref as ref
from fast_nnunet_amd import capi
from fast_nnunet_amd import postprocessing as pp
from fast_nnunet_amd.postprocessing import (fill_holes_in_segmentation, remove_all_but_largest_component_from_segmentation,
                                            remove_small_components_from_segmentation)

LARGEST, SMALL, HOLES = (remove_all_but_largest_component_from_segmentation, remove_small_components_from_segmentation,
                         fill_holes_in_segmentation)


# ---- the reference model on hand-made maps ----------------------------------------------------------------------------
@pytest.mark.parametrize('case', ref.hole_cases(), ids=lambda c: c[0])
def test_hole_model_on_hand_made_maps(case):
    _, seg, kw, want = case
    before = seg.copy()
    got = ref.fill_holes_ref(seg, **kw)
    assert np.array_equal(seg, before) and got.dtype == seg.dtype
    assert np.array_equal(got, want)


@pytest.mark.parametrize('case', ref.small_cases(), ids=lambda c: c[0])
def test_small_component_model_on_hand_made_maps(case):
    _, seg, kw, want = case
    before = seg.copy()
    got = ref.remove_small_ref(seg, **kw)
    assert np.array_equal(seg, before) and got.dtype == seg.dtype
    assert np.array_equal(got, want)


def test_hole_model_depth_one_volume_has_no_hole_and_the_plane_has():
    ring = np.zeros((5, 5), np.uint8)
    ring[1:4, 1:4] = 1; ring[2, 2] = 0
    assert ref.fill_holes_ref(ring, [1])[2, 2] == 1
    assert np.array_equal(ref.fill_holes_ref(ring[None], [1]), ring[None])       # every voxel of (1, Y, Z) is on a border


# ---- the pass planner -------------------------------------------------------------------------------------------------
def test_planner_each_kind_is_a_pass_of_its_own_in_order():
    def other(seg):
        return seg
    fns = [LARGEST, SMALL, HOLES, other, SMALL]
    kws = [{'labels_or_regions': [1, 2]}, {'labels_or_regions': 1, 'min_size': 5}, {'labels_or_regions': 2}, {},
           {'labels_or_regions': 2, 'min_size': 3}]
    passes = pp.plan_passes(fns, kws)
    assert [k for k, _ in passes] == ['gpu', 'gpu_small', 'gpu_holes', 'host', 'gpu_small']
    assert passes[1][1] == [(frozenset({1}), 0, 1, 5)]
    assert passes[2][1] == [(frozenset({2}), 0, 2, 2)]                          # fill_label defaults to the only label
    assert passes[3][1] == 3


def test_planner_joins_consecutive_small_component_steps_under_the_disjointness_rule():
    kws = [{'labels_or_regions': i, 'min_size': 10 * i} for i in (1, 2, 3)]
    (kind, body), = pp.plan_passes([SMALL] * 3, kws)
    assert kind == 'gpu_small' and [(sorted(s), bg, k, m) for s, bg, k, m in body] == [([1], 0, 0, 10), ([2], 0, 1, 20), ([3], 0, 2, 30)]
    # overlapping sets, another background, a set that holds the background, another connectivity: a new pass each
    assert len(pp.plan_passes([SMALL] * 2, [{'labels_or_regions': [(1, 2)], 'min_size': 4}, {'labels_or_regions': 2, 'min_size': 4}])) == 2
    assert len(pp.plan_passes([SMALL] * 2, [{'labels_or_regions': 1, 'min_size': 4},
                                            {'labels_or_regions': 2, 'min_size': 4, 'background_label': 3}])) == 2
    assert len(pp.plan_passes([SMALL] * 2, [{'labels_or_regions': 1, 'min_size': 4}, {'labels_or_regions': [(0, 2)], 'min_size': 4}])) == 2
    assert len(pp.plan_passes([SMALL] * 2, [{'labels_or_regions': 1, 'min_size': 4},
                                            {'labels_or_regions': 2, 'min_size': 4, 'connectivity': 6}])) == 2
    # ... and a largest-component step never joins a small-component pass, nor two hole steps each other
    assert [k for k, _ in pp.plan_passes([SMALL, LARGEST, SMALL], [{'labels_or_regions': 1, 'min_size': 4}, {'labels_or_regions': 2},
                                                                   {'labels_or_regions': 3, 'min_size': 4}])] == ['gpu_small', 'gpu', 'gpu_small']
    assert len(pp.plan_passes([HOLES] * 2, [{'labels_or_regions': 1}, {'labels_or_regions': 2}])) == 2


def test_planner_per_member_step_gives_one_set_per_member_in_one_pass():
    (kind, body), = pp.plan_passes([SMALL], [{'labels_or_regions': [1, (2, 3), 4], 'min_size': [5, 6, 7], 'per_member': True}])
    assert kind == 'gpu_small' and [(sorted(s), m) for s, _, _, m in body] == [([1], 5), ([2, 3], 6), ([4], 7)]
    (kind, body), = pp.plan_passes([SMALL], [{'labels_or_regions': [1, (2, 3), 4], 'min_size': 5}])
    assert [(sorted(s), m) for s, _, _, m in body] == [([1, 2, 3, 4], 5)]


def test_fused_small_component_passes_equal_sequential_steps_on_the_model():
    rng = np.random.default_rng(5)
    seg = rng.integers(0, 5, (9, 10, 11)).astype(np.uint8)
    for kws in ([{'labels_or_regions': i, 'min_size': 2 + i} for i in range(1, 5)],
                [{'labels_or_regions': [(1, 2)], 'min_size': 9}, {'labels_or_regions': 2, 'min_size': 3}, {'labels_or_regions': 3, 'min_size': 3}],
                [{'labels_or_regions': 1, 'min_size': 3, 'background_label': 2}, {'labels_or_regions': 3, 'min_size': 3, 'background_label': 2}]):
        want = ref.apply_ref(seg, [('small', kw) for kw in kws])
        got = seg
        for _, body in pp.plan_passes([SMALL] * len(kws), kws):
            base, got = got, np.copy(got)
            for s, bg, _, m in body:                                             # one labelling of the pass's input per set
                got[ref.small_components_of_set(base, sorted(s), m)] = bg
        assert np.array_equal(got, want)


# ---- the pkl loader -----------------------------------------------------------------------------------------------------
def test_pkl_loader_admits_the_two_steps_under_this_package_and_nothing_else():
    kws = [{'labels_or_regions': [1], 'min_size': 50, 'connectivity': 6}, {'labels_or_regions': [(1, 2)], 'fill_label': 1}]
    fns, got = pp.load_postprocessing_pkl(pickle.dumps(([SMALL, HOLES], kws)))
    assert fns == [SMALL, HOLES] and got == kws
    assert SMALL.__module__ == 'fast_nnunet_amd.postprocessing'
    with pytest.raises(pickle.UnpicklingError):
        pp.load_postprocessing_pkl(pickle.dumps(([pp.label_set], [{}])))        # another name of the same module
    with pytest.raises(pickle.UnpicklingError):
        pp.load_postprocessing_pkl(pickle.dumps(([os.system], [{}])))


# ---- refusals from the arguments alone, no GPU present ----------------------------------------------------------------------
SEG8 = np.zeros((3, 4, 5), np.uint8)
SEG16 = np.zeros((3, 4, 5), np.uint16)


@pytest.mark.parametrize('name,call,word', [
    ('connectivity-18', lambda: remove_small_components_from_segmentation(SEG8, [1], 5, connectivity=18), 'connectivity'),
    ('connectivity-none', lambda: remove_small_components_from_segmentation(SEG8, [1], 5, connectivity=None), 'connectivity'),
    ('min_size-negative', lambda: remove_small_components_from_segmentation(SEG8, [1], -1), 'min_size'),
    ('min_size-fraction', lambda: remove_small_components_from_segmentation(SEG8, [1], 2.5), 'min_size'),
    ('min_size-text', lambda: remove_small_components_from_segmentation(SEG8, [1], '5'), 'min_size'),
    ('min_size-count', lambda: remove_small_components_from_segmentation(SEG8, [1, 2], [5], per_member=True), 'min_size'),
    ('members-overlap', lambda: remove_small_components_from_segmentation(SEG8, [(1, 2), 2], 5, per_member=True), 'labels_or_regions'),
    ('small-background-u8', lambda: remove_small_components_from_segmentation(SEG8, [1], 5, background_label=256), 'background_label'),
    ('small-background-negative', lambda: remove_small_components_from_segmentation(SEG16, [1], 5, background_label=-1), 'background_label'),
    ('fill-missing', lambda: fill_holes_in_segmentation(SEG8, [(1, 2)]), 'fill_label'),
    ('fill-missing-list', lambda: fill_holes_in_segmentation(SEG8, [1, 2]), 'fill_label'),
    ('fill-u8', lambda: fill_holes_in_segmentation(SEG8, [1], fill_label=300), 'fill_label'),
    ('fill-u16', lambda: fill_holes_in_segmentation(SEG16, [1], fill_label=65536), 'fill_label'),
    ('fill-negative', lambda: fill_holes_in_segmentation(SEG8, [1], fill_label=-2), 'fill_label'),
    ('holes-background-u8', lambda: fill_holes_in_segmentation(SEG8, [1], background_label=256), 'background_label'),
    ('fill-equals-background', lambda: fill_holes_in_segmentation(SEG8, [1], fill_label=3, background_label=3), 'fill_label'),
    ('fill-default-equals-background', lambda: fill_holes_in_segmentation(SEG8, [1], background_label=1), 'background_label'),
    ('through-apply', lambda: pp.apply_postprocessing(SEG8, [SMALL], [{'labels_or_regions': 1, 'min_size': 3, 'connectivity': 8}]),
     'connectivity'),
], ids=lambda v: v if isinstance(v, str) and '-' in v else None)
def test_python_refuses_bad_arguments_before_any_gpu_call(name, call, word):
    with pytest.raises(ValueError, match=word):
        call()


def test_a_uint16_map_takes_labels_above_255():
    """No refusal where the dtype holds the label: the call goes on to ask for a GPU, and runs where there is one."""
    import torch
    if torch.cuda.is_available():
        assert np.array_equal(fill_holes_in_segmentation(SEG16, [300], background_label=256), SEG16)
        return
    with pytest.raises(RuntimeError, match='no GPU'):
        fill_holes_in_segmentation(SEG16, [300], background_label=256)


def _entry_text(fn, *args):
    lib = capi.load_library()
    code = getattr(lib, fn)(*args)
    return code, lib.fnn_last_error(None).decode()


def test_c_entries_refuse_bad_arguments_without_a_gpu():
    shape, table = (C.c_int64 * 3)(2, 2, 2), (C.c_int32 * 3)(-1, 0, 1)
    buf, sizes = (C.c_uint8 * 8)(), (C.c_int64 * 2)(3, 3)
    U8 = capi.FNN_LABEL_U8
    fn = 'fnn_remove_small_components'
    good = [buf, U8, shape, table, 3, 2, 0, sizes, 26, None, None]

    def bad(i, v):
        return good[:i] + [v] + good[i + 1:]
    for conn in (18, 0, 8, -6):
        assert _entry_text(fn, *bad(8, conn)) == (capi.FNN_E_UNSUPPORTED, fn + ': connectivity must be 6 or 26')
    assert _entry_text(fn, *bad(7, None)) == (capi.FNN_E_INVALID, 'NULL min_size')
    assert _entry_text(fn, *bad(2, None)) == (capi.FNN_E_INVALID, 'NULL shape')
    assert _entry_text(fn, *bad(1, 7)) == (capi.FNN_E_INVALID, 'unknown label dtype')
    assert _entry_text(fn, *bad(6, 256)) == (capi.FNN_E_INVALID, 'background_label outside the label dtype')
    assert _entry_text(fn, *bad(3, (C.c_int32 * 3)(-1, 2, 0))) == (capi.FNN_E_INVALID, 'group_of_label entry outside [-1, n_groups)')
    assert _entry_text(fn, *bad(2, (C.c_int64 * 3)(2048, 2048, 1024))) == (capi.FNN_E_UNSUPPORTED, fn + ': more than 2^31 - 1 voxels')
    assert _entry_text(fn, *good) == (capi.FNN_E_INVALID, fn + ' needs a device label map (no CPU path)')
    assert _entry_text(fn, *bad(0, None)) == (capi.FNN_E_INVALID, fn + ' needs a device label map (no CPU path)')
    removed = (C.c_int64 * 2)(9, 9)
    assert getattr(capi.load_library(), fn)(None, U8, (C.c_int64 * 3)(0, 4, 4), table, 3, 2, 0, sizes, 6, removed, None) == 0
    assert list(removed) == [0, 0]                                             # a zero-size volume: zeros, nothing else

    fn = 'fnn_fill_holes'
    member = (C.c_int32 * 3)(-1, 0, -1)
    good = [buf, U8, shape, member, 3, 0, 1, 7, None, None]
    assert _entry_text(fn, *bad(2, None)) == (capi.FNN_E_INVALID, 'NULL shape')
    assert _entry_text(fn, *bad(1, 7)) == (capi.FNN_E_INVALID, 'unknown label dtype')
    assert _entry_text(fn, *bad(5, 256)) == (capi.FNN_E_INVALID, 'background_label outside the label dtype')
    assert _entry_text(fn, *bad(6, 256)) == (capi.FNN_E_INVALID, 'fill_label outside the label dtype')
    assert _entry_text(fn, *bad(6, -1)) == (capi.FNN_E_INVALID, 'fill_label outside the label dtype')
    assert _entry_text(fn, *bad(6, 0)) == (capi.FNN_E_INVALID, 'fill_label equals background_label')
    for axes in (0, 8, -1):
        assert _entry_text(fn, *bad(7, axes)) == (capi.FNN_E_INVALID, 'border_axes must be 1..7 (bit a: axis a has borders)')
    assert _entry_text(fn, *bad(2, (C.c_int64 * 3)(2, -1, 2))) == (capi.FNN_E_INVALID, 'negative shape')
    assert _entry_text(fn, *bad(3, None)) == (capi.FNN_E_INVALID, 'bad label-set table')
    assert _entry_text(fn, *bad(3, (C.c_int32 * 3)(-1, 1, -1))) == (capi.FNN_E_INVALID, 'group_of_label entry outside [-1, 0]')
    assert _entry_text(fn, *bad(2, (C.c_int64 * 3)(2048, 2048, 1024))) == (capi.FNN_E_UNSUPPORTED, fn + ': more than 2^31 - 1 voxels')
    assert _entry_text(fn, *good) == (capi.FNN_E_INVALID, fn + ' needs a device label map (no CPU path)')
    filled = C.c_int64(9)
    assert getattr(capi.load_library(), fn)(None, U8, (C.c_int64 * 3)(4, 0, 4), member, 3, 0, 1, 7, C.byref(filled), None) == 0
    assert filled.value == 0
