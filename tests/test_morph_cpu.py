"""Binary morphology without a GPU: the scipy restatement (tests/morph_ref.py) on hand-made maps whose answer is written out,
the claim the device iterates on (n iterations are n one-step passes over a map padded with the border value), the pass
planner, the pkl loader, and every refusal that comes from the arguments alone (ValueError naming the argument)."""
import os
import pickle

import numpy as np
import pytest
from scipy import ndimage

import morph_ref as ref
from fast_nnunet_amd import capi
from fast_nnunet_amd import postprocessing as pp
from fast_nnunet_amd.postprocessing import (binary_closing_in_segmentation, binary_dilation_in_segmentation,
                                            binary_erosion_in_segmentation, binary_opening_in_segmentation,
                                            fill_holes_in_segmentation, remove_all_but_largest_component_from_segmentation,
                                            remove_small_components_from_segmentation)

DILATE, ERODE, OPEN, CLOSE = (binary_dilation_in_segmentation, binary_erosion_in_segmentation, binary_opening_in_segmentation,
                              binary_closing_in_segmentation)
LARGEST, SMALL, HOLES = (remove_all_but_largest_component_from_segmentation, remove_small_components_from_segmentation,
                         fill_holes_in_segmentation)


# ---- the reference model on hand-made maps ----------------------------------------------------------------------------
@pytest.mark.parametrize('case', ref.cases(), ids=lambda c: c[0])
def test_model_on_hand_made_maps(case):
    _, op, seg, kw, want = case
    before = seg.copy()
    got = ref.morph_ref(seg, op, **kw)
    assert np.array_equal(seg, before) and got.dtype == seg.dtype
    assert np.array_equal(got, want)


def test_the_two_facts_the_label_rule_rests_on():
    """With border_value 0 scipy's closing is not extensive at the border, with 1 its opening is not anti-extensive."""
    m = np.zeros((6, 5, 5), bool)
    m[0:4, 1:4, 1:4] = True
    closed = ref.scipy_result(m, 'closing', border_value=0)
    assert (m & ~closed).any() and not (closed & ~m).any()
    opened = ref.scipy_result(m, 'opening', border_value=1)
    assert (opened & ~m).any()
    for op, b in (('closing', 1), ('opening', 0)):
        r = ref.scipy_result(m, op, border_value=b)
        assert not ((m & ~r).any() if op == 'closing' else (r & ~m).any())


def _one_step_passes(mask, op, n, rank, border):
    """n one-step passes over the map padded with the border value (opening: n erosions then n dilations, closing the reverse)."""
    st = ndimage.generate_binary_structure(mask.ndim, min(rank, mask.ndim))
    runs = {'dilation': 'd', 'erosion': 'e', 'opening': 'ed', 'closing': 'de'}[op]
    cur = mask
    for step in runs:
        for _ in range(n):
            padded = np.pad(cur, 1, constant_values=bool(border))
            fn = ndimage.binary_dilation if step == 'd' else ndimage.binary_erosion
            cur = fn(padded, structure=st, border_value=border)[(slice(1, -1),) * mask.ndim]
    return cur


@pytest.mark.parametrize('shape', [(5, 6, 7), (1, 6, 9), (7, 8)], ids=str)
def test_n_iterations_are_n_one_step_passes_over_a_padded_map(shape):
    rng = np.random.default_rng(34)
    for density in (0.2, 0.6, 0.9):
        mask = rng.random(shape) < density
        for op in ref.OPS:
            for conn, rank in ref.RANK.items():
                for n in (1, 2, 3):
                    for border in (0, 1):
                        assert np.array_equal(ref.scipy_result(mask, op, n, conn, border), _one_step_passes(mask, op, n, rank, border)), \
                            (op, conn, n, border, density)


# ---- the pass planner -------------------------------------------------------------------------------------------------
def test_planner_gives_one_morph_entry_per_step_in_order_between_other_kinds():
    def other(seg):
        return seg
    fns = [CLOSE, HOLES, OPEN, OPEN, other, DILATE, LARGEST, ERODE, SMALL]
    kws = [{'labels_or_regions': [1], 'iterations': 2}, {'labels_or_regions': 1}, {'labels_or_regions': [(1, 2)], 'connectivity': 26},
           {'labels_or_regions': 3}, {}, {'labels_or_regions': [(1, 2)], 'fill_label': 2, 'border_value': 1, 'background_label': 4},
           {'labels_or_regions': 1}, {'labels_or_regions': 2, 'connectivity': 18, 'iterations': 1024}, {'labels_or_regions': 1, 'min_size': 3}]
    passes = pp.plan_passes(fns, kws)
    assert [k for k, _ in passes] == ['gpu_morph', 'gpu_holes', 'gpu_morph', 'gpu_morph', 'host', 'gpu_morph', 'gpu', 'gpu_morph', 'gpu_small']
    M = pp.MorphParams
    assert passes[0][1] == [(frozenset({1}), 0, 0, M(capi.FNN_MORPH_CLOSE, 6, 2, 0, 1))]     # fill_label defaults to the only label
    assert passes[2][1] == [(frozenset({1, 2}), 0, 2, M(capi.FNN_MORPH_OPEN, 26, 1, 0, 0))]
    assert passes[3][1] == [(frozenset({3}), 0, 3, M(capi.FNN_MORPH_OPEN, 6, 1, 0, 0))]     # two steps never share an entry
    assert passes[5][1] == [(frozenset({1, 2}), 4, 5, M(capi.FNN_MORPH_DILATE, 6, 1, 1, 2))]
    assert passes[7][1] == [(frozenset({2}), 0, 7, M(capi.FNN_MORPH_ERODE, 18, 1024, 0, 0))]
    assert (capi.FNN_MORPH_DILATE, capi.FNN_MORPH_ERODE, capi.FNN_MORPH_OPEN, capi.FNN_MORPH_CLOSE) == (0, 1, 2, 3)


def test_planner_takes_a_host_step_that_cannot_be_hashed():
    class Step:
        __hash__ = None

        def __eq__(self, other):
            return False

        def __call__(self, seg):
            return seg
    step = Step()
    passes = pp.plan_passes([ERODE, step, DILATE], [{'labels_or_regions': 1}, {}, {'labels_or_regions': 1}])
    assert [k for k, _ in passes] == ['gpu_morph', 'host', 'gpu_morph'] and passes[1][1] == 1


def test_gpu_pass_keeps_its_earlier_fields_and_defaults():
    assert pp.GpuPass._fields[:6] == ('call', 'sets', 'background', 'min_size', 'connectivity', 'fill_label')
    p = pp.GpuPass('largest', [frozenset({1})], 0)
    assert (p.min_size, p.connectivity, p.fill_label, p.op, p.iterations, p.border_value) == ((), 26, 0, 0, 1, 0)
    kw = {'labels_or_regions': 5, 'iterations': 3, 'connectivity': 18, 'border_value': 1, 'fill_label': 6}
    (kind, body), = pp.plan_passes([CLOSE], [kw])
    assert pp._gpu_pass(kind, body, [kw]) == pp.GpuPass('morph', [frozenset({5})], 0, connectivity=18, fill_label=6,
                                                        op=capi.FNN_MORPH_CLOSE, iterations=3, border_value=1)


# ---- the pkl loader -----------------------------------------------------------------------------------------------------
def test_pkl_loader_admits_the_four_steps_under_this_package_and_nothing_else():
    fns = [DILATE, ERODE, OPEN, CLOSE]
    kws = [{'labels_or_regions': [1], 'iterations': 2, 'fill_label': 1}, {'labels_or_regions': [(1, 2)], 'connectivity': 26},
           {'labels_or_regions': 2, 'border_value': 1}, {'labels_or_regions': [1, 2], 'fill_label': 2, 'background_label': 0}]
    got_fns, got_kws = pp.load_postprocessing_pkl(pickle.dumps((fns, kws)))
    assert all(a is b for a, b in zip(got_fns, fns)) and len(got_fns) == 4 and got_kws == kws
    assert all(f.__module__ == 'fast_nnunet_amd.postprocessing' for f in fns)
    assert [k for k, _ in pp.plan_passes(got_fns, got_kws)] == ['gpu_morph'] * 4
    with pytest.raises(pickle.UnpicklingError):
        pp.load_postprocessing_pkl(pickle.dumps(([pp.plan_passes], [{}])))      # another name of the same module
    with pytest.raises(pickle.UnpicklingError):
        pp.load_postprocessing_pkl(pickle.dumps(([ndimage.binary_dilation], [{}])))
    with pytest.raises(pickle.UnpicklingError):
        pp.load_postprocessing_pkl(pickle.dumps(([os.system], [{}])))


# ---- refusals from the arguments alone, no GPU present ----------------------------------------------------------------------
SEG8 = np.zeros((3, 4, 5), np.uint8)
SEG16 = np.zeros((3, 4, 5), np.uint16)


@pytest.mark.parametrize('name,call,word', [
    ('iterations-0', lambda: DILATE(SEG8, [1], iterations=0), 'iterations'),
    ('iterations-negative', lambda: ERODE(SEG8, [1], iterations=-1), 'iterations'),
    ('iterations-1025', lambda: OPEN(SEG8, [1], iterations=1025), 'iterations'),
    ('iterations-fraction', lambda: CLOSE(SEG8, [1], iterations=1.5), 'iterations'),
    ('iterations-bool', lambda: CLOSE(SEG8, [1], iterations=True), 'iterations'),
    ('iterations-text', lambda: DILATE(SEG8, [1], iterations='2'), 'iterations'),
    ('connectivity-8', lambda: DILATE(SEG8, [1], connectivity=8), 'connectivity'),
    ('connectivity-none', lambda: ERODE(SEG8, [1], connectivity=None), 'connectivity'),
    ('connectivity-rank', lambda: OPEN(SEG8, [1], connectivity=3), 'connectivity'),
    ('border-2', lambda: CLOSE(SEG8, [1], border_value=2), 'border_value'),
    ('border-negative', lambda: ERODE(SEG8, [1], border_value=-1), 'border_value'),
    ('border-none', lambda: OPEN(SEG8, [1], border_value=None), 'border_value'),
    ('fill-missing-dilation', lambda: DILATE(SEG8, [(1, 2)]), 'fill_label'),
    ('fill-missing-closing', lambda: CLOSE(SEG8, [1, 2]), 'fill_label'),
    ('fill-u8', lambda: DILATE(SEG8, [1], fill_label=300), 'fill_label'),
    ('fill-u16', lambda: CLOSE(SEG16, [1], fill_label=65536), 'fill_label'),
    ('fill-negative', lambda: CLOSE(SEG8, [1], fill_label=-2), 'fill_label'),
    ('fill-equals-background', lambda: DILATE(SEG8, [1], fill_label=3, background_label=3), 'fill_label'),
    ('fill-default-equals-background', lambda: CLOSE(SEG8, [1], background_label=1), 'background_label'),
    ('background-u8', lambda: ERODE(SEG8, [1], background_label=256), 'background_label'),
    ('background-negative', lambda: OPEN(SEG16, [1], background_label=-1), 'background_label'),
    ('background-fraction', lambda: DILATE(SEG8, [1], background_label=0.5), 'background_label'),
    ('fill-for-erosion', lambda: pp.apply_postprocessing(SEG8, [ERODE], [{'labels_or_regions': 1, 'fill_label': 2}]), 'fill_label'),
    ('through-apply', lambda: pp.apply_postprocessing(SEG8, [HOLES, OPEN], [{'labels_or_regions': 1}, {'labels_or_regions': 1, 'iterations': 0}]),
     'iterations'),
    ('float-map', lambda: DILATE(SEG8.astype(np.float32), [1]), 'integer dtype'),
    ('label-too-large', lambda: ERODE(np.full((2, 2, 2), 70000, np.int32), [1]), '65535'),
], ids=lambda v: v if isinstance(v, str) and '-' in v else None)
def test_python_refuses_bad_arguments_before_any_gpu_call(name, call, word, monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)              # no GPU visible: a call that got that far says so
    with pytest.raises(ValueError, match=word):
        call()


def test_good_arguments_go_on_to_ask_for_a_gpu(monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    for call in (lambda: DILATE(SEG16, [300], iterations=1024, connectivity=18, border_value=1, background_label=256),
                 lambda: ERODE(SEG8, [(1, 2)], border_value=True), lambda: OPEN(SEG8.reshape(3, 20), 1, connectivity=26),
                 lambda: CLOSE(SEG8, [(1, 2)], fill_label=2)):
        with pytest.raises(RuntimeError, match='no GPU'):
            call()
