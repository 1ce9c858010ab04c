"""Connected-component postprocessing without a GPU: the postprocessing.pkl loader, the pass planner, and the CPU
restatement of the reference's rule that tests/test_gpu_postprocessing.py compares the device results against.

The rule (nnunetv2 remove_all_but_largest_component_from_segmentation -> acvl_utils remove_all_but_largest_component):
mask = seg in S; label the mask with full connectivity (26 neighbours in 3-D, 8 in 2-D); keep every component whose
size equals the largest; voxels of the mask outside them become background_label; the input stays as it is.
"""
import os
import pickle
import sys
import types

import numpy as np
import pytest
from scipy import ndimage


def _set_of(labels_or_regions):
    members = labels_or_regions if isinstance(labels_or_regions, list) else [labels_or_regions]
    out = set()
    for m in members:
        out.update([int(m)] if np.isscalar(m) else [int(v) for v in m])
    return sorted(out)


def keep_largest_ref(seg, labels_or_regions, background_label=0):
    """The rule restated with scipy (one component labelling of the whole mask)."""
    seg = np.asarray(seg)
    mask = np.isin(seg, _set_of(labels_or_regions))
    lab, n = ndimage.label(mask, structure=ndimage.generate_binary_structure(seg.ndim, seg.ndim))
    ret = np.copy(seg)
    if n == 0:
        return ret
    sizes = np.bincount(lab.ravel())[1:]
    keep = np.isin(lab, np.flatnonzero(sizes == sizes.max()) + 1)
    ret[mask & ~keep] = background_label
    return ret


def keep_largest_ref_boxed(seg, label, background_label=0, box=None):
    """The same for one label, labelled only inside its bounding box (every component of the label lies in it): fast on
    large maps with small labels.  ``box``: ndimage.find_objects(seg)[label - 1], if the caller has it."""
    ret = np.copy(seg)
    if box is None:
        boxes = ndimage.find_objects((seg == label).astype(np.uint8))
        box = boxes[0] if boxes else None
    if box is not None:
        ret[box] = keep_largest_ref(seg[box], [label], background_label)
    return ret


def apply_ref(seg, pp_fn_kwargs):
    for kw in pp_fn_kwargs:
        seg = keep_largest_ref(seg, kw['labels_or_regions'], kw.get('background_label', 0))
    return seg


# ---- the restatement on hand-made cases -----------------------------------------------------------------------------
def hand_cases():
    """(name, seg, labels_or_regions, background_label, expected) - expected written out by hand."""
    out = []
    a = np.zeros((4, 4, 4), np.uint8)
    a[0, 0, 0] = 1; a[1, 1, 1] = 1                        # touch only at a corner: one component
    a[3, 0, 3] = 1                                          # a singleton elsewhere
    e = a.copy(); e[3, 0, 3] = 0
    out.append(('corner', a, [1], 0, e))
    b = np.zeros((4, 6, 5), np.uint8)
    b[0, 0, 0:2] = 2; b[3, 5, 3:5] = 2; b[2, 0, 4] = 2      # two equal largest (2 voxels) and one smaller
    e = b.copy(); e[2, 0, 4] = 0
    out.append(('ties', b, [2], 0, e))
    c = np.zeros((5, 4, 3), np.uint8); c[1, 1, 1] = 3
    out.append(('empty_mask', c, [1], 0, c.copy()))
    d = np.full((4, 5, 6), 7, np.uint8)
    d[0, 0, 0:3] = 1; d[3, 4, 5] = 1
    e = d.copy(); e[3, 4, 5] = 7
    out.append(('background_7', d, [1], 7, e))
    f = np.zeros((6, 7), np.int64)                          # 2-D: 8-connectivity
    f[0, 0] = 1; f[1, 1] = 1; f[5, 6] = 1
    e = f.copy(); e[5, 6] = 0
    out.append(('2d_diagonal', f, [1], 0, e))
    g = np.zeros((3, 4, 4), np.uint8)                       # a region (tuple): labels 1 and 2 together
    g[0, 0, 0] = 1; g[0, 0, 1] = 2; g[2, 3, 3] = 2
    e = g.copy(); e[2, 3, 3] = 0
    out.append(('region', g, [(1, 2)], 0, e))
    return out


@pytest.mark.parametrize('case', hand_cases(), ids=lambda c: c[0])
def test_restatement_on_hand_made_cases(case):
    _, seg, lor, bg, want = case
    before = seg.copy()
    got = keep_largest_ref(seg, lor, bg)
    assert np.array_equal(seg, before)                      # the input is left unmodified
    assert got.dtype == seg.dtype and got.shape == seg.shape
    assert np.array_equal(got, want)


# ---- the postprocessing.pkl loader ----------------------------------------------------------------------------------
MOD = 'nnunetv2.postprocessing.remove_connected_components'
FN = 'remove_all_but_largest_component_from_segmentation'


def _reference_pickle(pp_fn_kwargs):
    """A pickle as nnunetv2's determine_postprocessing writes it, made with a stand-in module under that name."""
    names = ['nnunetv2', 'nnunetv2.postprocessing', MOD]
    saved = {n: sys.modules.get(n) for n in names}
    try:
        for n in names:
            sys.modules[n] = types.ModuleType(n)
        mod = sys.modules[MOD]

        def stand_in(segmentation, labels_or_regions, background_label=0):
            raise AssertionError('the stand-in is never called')
        stand_in.__module__ = MOD
        stand_in.__qualname__ = stand_in.__name__ = FN
        setattr(mod, FN, stand_in)
        return pickle.dumps(([stand_in] * len(pp_fn_kwargs), pp_fn_kwargs))
    finally:
        for n, m in saved.items():
            if m is None:
                sys.modules.pop(n, None)
            else:
                sys.modules[n] = m


def test_pkl_loader_reads_a_reference_pickle(tmp_path):
    from fast_nnunet_amd import postprocessing as pp
    kwargs = [{'labels_or_regions': [1, 2, 3]}] + [{'labels_or_regions': np.int64(i)} for i in (1, 2, 3)]
    kwargs.append({'labels_or_regions': [(1, 2)], 'background_label': np.int32(0)})
    blob = _reference_pickle(kwargs)
    assert MOD not in sys.modules
    path = os.path.join(tmp_path, 'postprocessing.pkl')
    with open(path, 'wb') as f:
        f.write(blob)
    fns, kws = pp.load_postprocessing_pkl(path)
    assert fns == [pp.remove_all_but_largest_component_from_segmentation] * 5
    assert [pp.label_set(k['labels_or_regions']) for k in kws] == [{1, 2, 3}, {1}, {2}, {3}, {1, 2}]
    assert kws[4]['background_label'] == 0
    assert pp.load_postprocessing_pkl(blob)[0] == fns


def test_pkl_loader_refuses_other_globals():
    from fast_nnunet_amd import postprocessing as pp
    blob = pickle.dumps(([os.system], [{'command': 'true'}]))
    with pytest.raises(pickle.UnpicklingError):
        pp.load_postprocessing_pkl(blob)

    class Evil:
        def __reduce__(self):
            return (os.system, ('true',))
    with pytest.raises(pickle.UnpicklingError):
        pp.load_postprocessing_pkl(pickle.dumps(([], [Evil()])))
    with pytest.raises(pickle.UnpicklingError):
        pp.load_postprocessing_pkl(pickle.dumps(([np.load], [{}])))


# ---- the pass planner -----------------------------------------------------------------------------------------------
def _fn():
    from fast_nnunet_amd import postprocessing as pp
    return pp.remove_all_but_largest_component_from_segmentation


def _plan(kwargs, fns=None):
    from fast_nnunet_amd import postprocessing as pp
    return pp.plan_passes(fns or [_fn()] * len(kwargs), kwargs)


def test_planner_whole_foreground_then_per_label_is_two_passes():
    kwargs = [{'labels_or_regions': list(range(1, 61))}] + [{'labels_or_regions': i} for i in range(1, 61)]
    passes = _plan(kwargs)
    assert len(passes) == 2
    assert [len(body) for _, body in passes] == [1, 60]
    assert [k for _, body in passes for _, _, k in body] == list(range(61))


def test_planner_overlapping_regions_are_sequential():
    passes = _plan([{'labels_or_regions': [(1, 2, 3)]}, {'labels_or_regions': [(2, 3)]}, {'labels_or_regions': [3]}])
    assert len(passes) == 3


def test_planner_mixed_backgrounds_do_not_fuse():
    passes = _plan([{'labels_or_regions': 1}, {'labels_or_regions': 2, 'background_label': 5}, {'labels_or_regions': 3}])
    assert len(passes) == 3


def test_planner_later_set_containing_the_background_does_not_fuse():
    passes = _plan([{'labels_or_regions': 1}, {'labels_or_regions': [(0, 2)]}])
    assert len(passes) == 2
    # ... but the background may be in the FIRST set of a pass
    passes = _plan([{'labels_or_regions': [(0, 2)]}, {'labels_or_regions': 1}])
    assert len(passes) == 1


def test_planner_runs_foreign_callables_on_their_own():
    def other(seg):
        return seg
    passes = _plan([{'labels_or_regions': 1}, {}, {'labels_or_regions': 2}], fns=[_fn(), other, _fn()])
    assert [kind for kind, _ in passes] == ['gpu', 'host', 'gpu']


def test_fused_passes_equal_sequential_steps_on_the_cpu_restatement():
    """The planner's condition is what makes one labelling per pass equal to the steps one after another: checked on
    the restatement (a pass = one labelling of the original map per set)."""
    from fast_nnunet_amd import postprocessing as pp
    rng = np.random.default_rng(3)
    seg = rng.integers(0, 5, (12, 13, 14)).astype(np.uint8)
    for kwargs in ([{'labels_or_regions': [1, 2, 3, 4]}] + [{'labels_or_regions': i} for i in range(1, 5)],
                   [{'labels_or_regions': [(1, 2, 3)]}, {'labels_or_regions': [(2, 3)]}, {'labels_or_regions': [3]}],
                   [{'labels_or_regions': 1, 'background_label': 2}, {'labels_or_regions': 3, 'background_label': 2}]):
        want = apply_ref(seg, kwargs)
        got = seg
        for _, body in pp.plan_passes([_fn()] * len(kwargs), kwargs):
            base = got
            got = np.copy(base)
            for s, bg, _ in body:
                one = keep_largest_ref(base, [tuple(s)], bg)
                changed = one != base
                got[changed] = one[changed]
        assert np.array_equal(got, want)


def test_values_outside_uint16_are_refused_before_any_gpu_work():
    from fast_nnunet_amd import postprocessing as pp
    with pytest.raises(ValueError):
        pp.remove_all_but_largest_component_from_segmentation(np.array([[[70000]]], np.int32), [1])
    with pytest.raises(ValueError):
        pp.remove_all_but_largest_component_from_segmentation(np.array([[[-1]]], np.int32), [1])
    with pytest.raises(ValueError):
        pp.remove_all_but_largest_component_from_segmentation(np.zeros((2, 2), np.float32), [1])


def test_library_refuses_bad_arguments_without_a_gpu():
    """Argument checks of fnn_keep_largest_components that come before any device work."""
    import ctypes as C
    from fast_nnunet_amd import capi
    lib = capi.load_library()
    shape = (C.c_int64 * 3)(2, 2, 2)
    table = (C.c_int32 * 2)(-1, 0)
    buf = (C.c_uint8 * 8)()
    # zero-size volume: nothing to do
    assert lib.fnn_keep_largest_components(None, capi.FNN_LABEL_U8, (C.c_int64 * 3)(0, 4, 4), table, 2, 1, 0, None, None) == 0
    # unknown dtype, background outside the dtype, host pointer, table entry out of range
    assert lib.fnn_keep_largest_components(buf, 7, shape, table, 2, 1, 0, None, None) == capi.FNN_E_INVALID
    assert lib.fnn_keep_largest_components(buf, capi.FNN_LABEL_U8, shape, table, 2, 1, 256, None, None) == capi.FNN_E_INVALID
    assert lib.fnn_keep_largest_components(buf, capi.FNN_LABEL_U8, shape, table, 2, 1, 0, None, None) == capi.FNN_E_INVALID
    assert lib.fnn_keep_largest_components(buf, capi.FNN_LABEL_U8, shape, table, 2, 0, 0, None, None) == capi.FNN_E_INVALID
    # more than 2^31 - 1 voxels
    big = (C.c_int64 * 3)(2048, 1024, 1024)
    assert lib.fnn_keep_largest_components(buf, capi.FNN_LABEL_U8, big, table, 2, 1, 0, None, None) == capi.FNN_E_UNSUPPORTED
