"""fnn_instance_overlaps and the lesion-wise metrics on one MI355X against tests/instance_ref.py: the whole record buffer,
the merged lists and every metric equal exactly - all are integers or floats derived from them.

The labelling works in tiles of 1024 voxels (8 x 8 x 16, or 4 x 16 x 16, or 1 x 32 x 32 for thin volumes) and the compaction
in blocks of 1024 raster-consecutive voxels; the shapes break both on every axis and at ragged ends."""
import json
import os

import numpy as np
import pytest
import torch

import instance_ref as ir

pytestmark = pytest.mark.gpu

SHAPES = [(9, 17, 35), (33, 34, 37), (1, 40, 70), (70, 40, 1), (3, 3, 3), (1, 1, 1)]
EIGHT = ['Dice', 'IoU', 'FP', 'TP', 'FN', 'TN', 'n_pred', 'n_ref']
SURFACE = ['HD', 'HD95', 'ASSD', 'NSD', 'n_surf_pred', 'n_surf_ref']
GUARD, SENTINEL = 8, -7


# ---- maps by construction: (ref, pred, disjoint regions, expected n_out or None)
def m_boxes(shape, dtype):
    """Boxes of label 1 at the low corner, across the middle and at the high corner of the reference; the prediction keeps the
    first, halves the second and has one of its own."""
    ref, pred = np.zeros(shape, dtype), np.zeros(shape, dtype)
    box = tuple(slice(0, max(1, n // 4)) for n in shape)
    ref[box] = pred[box] = 1
    n_ref, n_pred, n_pieces = 1, 1, 1
    if min(shape) >= 9:
        mid = tuple(slice(n // 2 - 2, n // 2 + 2) for n in shape)
        ref[mid] = 1
        pred[mid[0], mid[1], slice(shape[2] // 2 - 2, shape[2] // 2)] = 1
        ref[tuple(slice(n - 2, n) for n in shape)] = 1
        pred[shape[0] - 1, 0, shape[2] - 1] = 1
        n_ref, n_pred, n_pieces = 3, 3, 2
    return ref, pred, [1], (n_ref, n_pred, n_pieces)


def m_staircase(shape, dtype):
    """A one-voxel-thick diagonal from corner to corner whose voxels touch only by their corners: one component with 26- but
    not with 18-connectivity, across every tile border on its way.  The prediction lacks every fifth voxel."""
    ref, pred = np.zeros(shape, dtype), np.zeros(shape, dtype)
    steps = min(shape)
    idx = tuple(np.arange(steps) for _ in shape)
    if steps == 1:                                                      # a thin volume: the diagonal of its plane
        long_axes = [a for a in range(3) if shape[a] > 1]
        steps = min((shape[a] for a in long_axes), default=1)
        idx = tuple(np.arange(steps) if a in long_axes else np.zeros(steps, int) for a in range(3))
    ref[idx] = 2
    pred[idx] = 2
    cut = np.arange(4, steps, 5)
    pred[tuple(i[cut] for i in idx)] = 0
    runs = len(cut) + (1 if steps - 1 not in cut else 0) if steps > 4 else 1
    return ref, pred, [2], (1, runs, runs)


def m_interleaved(shape, dtype):
    """Two labels plane by plane along the slowest axis with more than one plane: every voxel touches the other label, and
    they must not merge.  The prediction is the reference."""
    axis = next((a for a in range(3) if shape[a] > 1), 0)
    planes = np.arange(shape[axis]) % 2 + 1
    ref = np.zeros(shape, dtype) + planes.reshape([-1 if a == axis else 1 for a in range(3)]).astype(dtype)
    n = shape[axis]
    return ref, ref.copy(), [1, 2], (n, n, n)


def m_ring(shape, dtype):
    at = (shape[0] // 2, shape[1] - 9, shape[2] - 9)
    ref, pred = ir.ring_and_arcs(shape, at, 1, dtype)
    return ref, pred, [1], (1, 2, 4)


def m_sparse(shape, dtype):
    labels = (1, 2, 300) if dtype == np.uint16 else (1, 2, 3)
    ref, pred = ir.sparse_pair(shape, sum(shape), labels=labels, dtype=dtype)
    return ref, pred, list(labels), None


def m_sparse_regions(shape, dtype):
    labels = (1, 2, 300) if dtype == np.uint16 else (1, 2, 3)
    ref, pred = ir.sparse_pair(shape, 7 + sum(shape), density=0.05, labels=labels, dtype=dtype)
    return ref, pred, [(labels[0], labels[2]), labels[1]], None


MAPS = {'boxes': m_boxes, 'staircase': m_staircase, 'interleaved': m_interleaved, 'ring': m_ring, 'sparse': m_sparse,
        'sparse_regions': m_sparse_regions}
RING_SHAPES = [s for s in SHAPES if s[1] >= 9 and s[2] >= 9]
CASES = [(name, shape, dtype) for name in MAPS for shape in (RING_SHAPES if name == 'ring' else SHAPES) for dtype in (np.uint8, np.uint16)]
_cache = {}


def case(name, shape, dtype):
    """(ref, pred, regions, expected n_out, yardstick n_out, yardstick records), computed once and left unchanged."""
    key = (name, shape, np.dtype(dtype).name)
    if key not in _cache:
        ref, pred, regions, counts = MAPS[name](shape, dtype)
        _cache[key] = (ref, pred, regions, counts) + ir.records(ref, pred, regions)
        _cache[key][5].setflags(write=False)
    return _cache[key]


def table_of(regions):
    sets = [list(r) if isinstance(r, tuple) else [r] for r in regions]
    table = np.full(max(v for s in sets for v in s) + 1, -1, np.int32)
    for g, s in enumerate(sets):
        table[s] = g
    return table


def device_records(ref, pred, regions, cap):
    """One call with room for ``cap`` records between guards of a sentinel: (n_out, the cap records, guards untouched)."""
    from fast_nnunet_amd import capi
    dev = torch.device('cuda', 0)
    u16 = ref.dtype != np.uint8
    as_t = lambda a: torch.from_numpy(a.astype(np.int16 if u16 else np.uint8)).to(dev)                  # (astype copies)
    d_ref, d_pred = as_t(ref), as_t(pred)
    buf = torch.full(((cap + 2 * GUARD) * 3,), SENTINEL, dtype=torch.int32, device=dev)
    n_out = capi.instance_overlaps_call(d_ref.data_ptr(), d_pred.data_ptr(), u16, ref.shape, table_of(regions), len(regions),
                                        buf.data_ptr() + GUARD * 12, cap, torch.cuda.current_stream(dev).cuda_stream)
    host = buf.cpu().numpy().reshape(-1, 3)
    guards_ok = bool((host[:GUARD] == SENTINEL).all() and (host[GUARD + cap:] == SENTINEL).all())
    return n_out, host[GUARD:GUARD + cap], guards_ok


@pytest.mark.parametrize('name,shape,dtype', CASES, ids=[f'{n}-{"x".join(map(str, s))}-{np.dtype(d).name}' for n, s, d in CASES])
def test_records_equal_the_yardsticks(name, shape, dtype):
    from fast_nnunet_amd import evaluation as ev
    ref, pred, regions, counts, want_n, want = case(name, shape, dtype)
    if counts is not None:
        assert tuple(want_n) == counts                                  # known by construction, without scipy's count
    total = int(want_n.sum())
    n_out, got, guards_ok = device_records(ref, pred, regions, total)
    assert guards_ok and list(n_out) == list(want_n)
    assert np.array_equal(got, want)
    # invariants: roots ascend; per group the sizes add up to the voxel counts of fnn_confusion_counts
    a, b = int(n_out[0]), int(n_out[0] + n_out[1])
    for part in (got[:a], got[a:b]):
        assert np.all(np.diff(part[:, 1]) > 0)
    values = sorted(v for r in regions for v in (r if isinstance(r, tuple) else (r,)))
    counted = ev.metrics_from_counts(ev.confusion_counts(ref, [pred], values)[0], regions)
    piece_group = got[a:b, 0][np.searchsorted(got[a:b, 1], got[b:, 0])]
    for g, r in enumerate(regions):
        assert got[:a][got[:a, 0] == g, 2].sum() == counted[r]['n_ref']
        assert got[a:b][got[a:b, 0] == g, 2].sum() == counted[r]['n_pred']
        assert got[b:][piece_group == g, 2].sum() == counted[r]['TP']
    again = device_records(ref, pred, regions, total)
    assert again[1].tobytes() == got.tobytes()                          # the same bytes on every run
    if total:
        n_short, untouched, guards_ok = device_records(ref, pred, regions, total - 1)
        assert guards_ok and list(n_short) == list(want_n) and (untouched == SENTINEL).all()


LATTICE = 40


def lattice():
    key = 'lattice'
    if key not in _cache:
        ref = np.zeros((LATTICE,) * 3, np.uint8)
        ref[::2, ::2, ::2] = 1
        _cache[key] = (ref, np.roll(ref, 2, axis=0).copy())
    return _cache[key]


def test_a_lattice_of_8000_one_voxel_components_goes_through_the_second_call():
    from fast_nnunet_amd import evaluation as ev
    ref, pred = lattice()
    calls, calls_small = [], []
    got = ev.instance_overlaps(ref, pred, [1], calls_made=calls)[1]
    small = ev.instance_overlaps(ref, pred, [1], first_capacity=16, calls_made=calls_small)[1]
    assert calls == [1] and calls_small == [2]
    ones, index = np.ones(8000, np.int64), np.arange(8000, dtype=np.int64)
    for lists in (got, small):
        assert np.array_equal(lists['ref_sizes'], ones) and np.array_equal(lists['pred_sizes'], ones)
        assert np.array_equal(lists['pairs'], np.stack([index, index, ones], axis=1))
    m = ev.compute_instance_metrics(ref, pred, [1])[1]
    assert (m['n_inst_ref'], m['inst_TP'], m['inst_FP'], m['PQ']) == (8000, 8000, 0, 1.0)


# ---- regions and labels
def regions_case():
    key = 'regions'
    if key not in _cache:
        ref, pred = ir.sparse_pair((17, 18, 35), 5, density=0.06)
        _cache[key] = (ref, pred)
    return _cache[key]


def same_lists(got, want):
    return all(got[k].dtype == np.int64 and np.array_equal(got[k], want[k]) for k in ('ref_sizes', 'pred_sizes', 'pairs'))


def test_nested_regions_take_one_call_each_and_33_labels_one():
    from fast_nnunet_amd import evaluation as ev
    ref, pred = regions_case()
    nested, calls = [(1, 2, 3), (2, 3), 3], []
    got = ev.instance_overlaps(ref, pred, nested, calls_made=calls)
    assert calls == [1, 1, 1] and list(got) == nested
    assert all(same_lists(got[r], ir.overlaps(ref, pred, r)) for r in nested)
    rng = np.random.default_rng(33)
    many = (rng.integers(1, 34, ref.shape) * (rng.random(ref.shape) < 0.2)).astype(np.uint8)
    many_pred = np.roll(many, 1, axis=1)
    labels, calls = list(range(1, 34)), []
    got = ev.instance_overlaps(many, many_pred, labels, calls_made=calls)
    assert calls == [1]
    assert all(same_lists(got[r], ir.overlaps(many, many_pred, r)) for r in labels)


@pytest.mark.parametrize('empty', ['ref', 'pred', 'both'])
def test_empty_sides(empty):
    from fast_nnunet_amd import evaluation as ev
    ref, pred = (a.copy() for a in regions_case())
    if empty in ('ref', 'both'):
        ref[:] = 0
    if empty in ('pred', 'both'):
        pred[:] = 0
    got, want = ev.compute_instance_metrics(ref, pred, [1, (2, 3)]), ir.case_metrics(ref, pred, [1, (2, 3)])
    for r in want:
        assert list(got[r]) == list(ev.INSTANCE_KEYS)
        assert all(ir.same_value(got[r][k], want[r][k]) for k in ir.KEYS), (r, got[r], want[r])
    assert np.isnan(got[1]['PQ']) == (empty == 'both')


def test_a_device_tensor_a_numpy_array_and_a_leading_axis():
    from fast_nnunet_amd import evaluation as ev
    ref, pred = regions_case()
    want = {r: ir.overlaps(ref, pred, r) for r in (1, 2, 3)}
    d_ref, d_pred = torch.from_numpy(ref).cuda(), torch.from_numpy(pred).cuda()
    wide = torch.from_numpy(pred.astype(np.int64))
    for a, b in ((ref, pred), (d_ref, d_pred), (d_ref[None], pred[None]), (ref, wide)):
        got = ev.instance_overlaps(a, b, [1, 2, 3])
        assert all(same_lists(got[r], want[r]) for r in want)
    assert torch.equal(d_ref.cpu(), torch.from_numpy(ref)) and torch.equal(d_pred.cpu(), torch.from_numpy(pred))
    with pytest.raises(ValueError, match='shape mismatch'):
        ev.instance_overlaps(ref, pred[:-1], [1])


# ---- through the layers
def test_compute_metrics_appends_the_keys_behind_the_others():
    from fast_nnunet_amd import evaluation as ev
    ref, pred = regions_case()
    regions = [1, (2, 3)]
    want = ir.case_metrics(ref, pred, regions)
    off = ev.compute_metrics(ref[None], pred[None], regions)['metrics']
    on = ev.compute_metrics(ref[None], pred[None], regions, instance_metrics=True)['metrics']
    both = ev.compute_metrics(ref, pred, regions, instance_metrics=True, surface_metrics=True, spacing=(1.0, 1.0, 1.0))['metrics']
    surf = ev.compute_metrics(ref, pred, regions, surface_metrics=True, spacing=(1.0, 1.0, 1.0))['metrics']
    for r in regions:
        assert list(off[r]) == EIGHT
        assert list(on[r]) == EIGHT + list(ev.INSTANCE_KEYS)
        assert list(both[r]) == EIGHT + SURFACE + list(ev.INSTANCE_KEYS)
        assert all(ir.same_value(on[r][k], off[r][k]) and ir.same_value(both[r][k], off[r][k]) for k in EIGHT)
        assert all(ir.same_value(both[r][k], surf[r][k]) for k in SURFACE)
        assert all(ir.same_value(on[r][k], want[r][k]) and ir.same_value(both[r][k], want[r][k]) for k in ir.KEYS)
    with pytest.raises(ValueError, match='instance metrics are refused together with an ignore label'):
        ev.compute_metrics(ref, pred, [1], ignore_label=2, instance_metrics=True)


def test_compute_metrics_on_arrays_with_its_summary(tmp_path):
    from fast_nnunet_amd import evaluation as ev
    ref, pred = regions_case()
    regions = [1, (2, 3)]
    out = os.path.join(tmp_path, 's.json')
    summary = ev.compute_metrics_on_arrays([ref, ref], [pred, ref], regions, output_file=out, instance_metrics=True)
    wants = [ir.case_metrics(ref, pred, regions), ir.case_metrics(ref, ref, regions)]
    loaded = ev.load_summary_json(out)
    for r in regions:
        for k in ir.KEYS:
            assert all(ir.same_value(c['metrics'][r][k], w[r][k]) for c, w in zip(summary['metric_per_case'], wants))
            assert ir.same_value(summary['mean'][r][k], np.nanmean([float(w[r][k]) for w in wants]))
            assert ir.same_value(loaded['mean'][r][k], summary['mean'][r][k])
    assert wants[1][1]['PQ'] == 1.0 and wants[1][1]['inst_F1'] == 1.0


FOLDER_SHAPE, LABELS = (9, 20, 31), [1, 2, 3]


def _write(rw, folder, maps):
    os.makedirs(folder, exist_ok=True)
    for i, m in enumerate(maps):
        rw.write_seg(m, os.path.join(folder, f'case_{i}.nii.gz'), {'nibabel_stuff': {'original_affine': np.diag([1.5, 2.0, 0.5, 1.0])}})


def _numpy_case(ref, pred, labels):
    from fast_nnunet_amd import evaluation as ev
    values = ev.count_classes(labels)
    cls = lambda a: np.where(np.isin(a, values), np.searchsorted(values, a), len(values)).reshape(-1)
    counts = np.zeros((len(values) + 1,) * 2, np.int64)
    np.add.at(counts, (cls(ref), cls(pred)), 1)
    return ev.metrics_from_counts(counts, labels)


def test_folder_summary_carries_the_means_and_is_unchanged_without_the_flag(tmp_path):
    from fast_nnunet_amd import evaluation as ev
    from fast_nnunet_amd.imageio import NiftiIO
    pairs = [ir.sparse_pair(FOLDER_SHAPE, 40 + k, density=0.06) for k in range(3)]
    pairs[1][1][pairs[1][1] == 2] = 0                                   # a label missing in one prediction
    refs, preds = [p[0] for p in pairs], [p[1] for p in pairs]
    fr, fp = os.path.join(tmp_path, 'ref'), os.path.join(tmp_path, 'pred')
    _write(NiftiIO(), fr, refs), _write(NiftiIO(), fp, preds)
    on, off = os.path.join(tmp_path, 'on.json'), os.path.join(tmp_path, 'off.json')
    ev.compute_metrics_on_folder_simple(fr, fp, LABELS, on, instance_metrics=True)
    ev.compute_metrics_on_folder_simple(fr, fp, LABELS, off)
    wants = [ir.case_metrics(r, p, LABELS) for r, p in pairs]
    got = ev.load_summary_json(on)
    for r in LABELS:
        for k in ir.KEYS:
            vals = [float(w[r][k]) for w in wants]
            assert all(ir.same_value(c['metrics'][r][k], v) for c, v in zip(got['metric_per_case'], vals)), (r, k)
            mean = np.nan if all(np.isnan(v) for v in vals) else float(np.nanmean(vals))
            assert ir.same_value(got['mean'][r][k], mean), (r, k)
    assert np.isnan(wants[1][2]['inst_precision']) and 'PQ' in got['foreground_mean']
    # without the flag: the bytes of a summary built from numpy counts by the host half alone, which this feature leaves as it was
    expected = os.path.join(tmp_path, 'expected.json')
    cases = [ev.case_result(_numpy_case(r, p, LABELS), os.path.join(fr, f'case_{i}.nii.gz'), os.path.join(fp, f'case_{i}.nii.gz'))
             for i, (r, p) in enumerate(pairs)]
    ev.save_summary_json(ev.aggregate(cases, LABELS), expected)
    assert open(off, 'rb').read() == open(expected, 'rb').read()
    with open(off) as f:
        assert sorted(json.load(f)['mean']['1']) == sorted(EIGHT)
