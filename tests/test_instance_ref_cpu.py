"""The host half of the lesion-wise metrics without a GPU: instance_metrics_of on hand-made lists with known answers and
against tests/instance_ref.py on small maps, the merge of the device's records, the plan of the calls, the flag through
compute_metrics with both device halves replaced by numpy, and the keys through aggregate and summary.json."""
import math
import os

import numpy as np
import pytest

import instance_ref as ir
from fast_nnunet_amd import capi
from fast_nnunet_amd import evaluation as ev

EIGHT = ['Dice', 'IoU', 'FP', 'TP', 'FN', 'TN', 'n_pred', 'n_ref']
NAN = float('nan')


def check(got, **want):
    assert tuple(got) == ev.INSTANCE_KEYS
    for k, v in got.items():
        assert isinstance(v, np.float64 if k in ('inst_recall', 'inst_precision', 'inst_F1', 'PQ', 'SQ', 'RQ') else np.int64), (k, type(v))
    for k, v in want.items():
        assert ir.same_value(got[k], v), (k, got[k], v)


def test_the_keys_are_the_table_of_the_definitions():
    assert ev.INSTANCE_KEYS == ir.KEYS == ('n_inst_ref', 'n_inst_pred', 'inst_TP', 'inst_FN', 'inst_FP', 'inst_recall', 'inst_precision',
                                           'inst_F1', 'FN_inst_vox', 'FP_inst_vox', 'PQ', 'SQ', 'RQ')


def test_one_lesion_hit_by_two_predicted_blobs():
    # |R| = 10; P_0 = 4 voxels, 3 inside; P_1 = 5 voxels, 5 inside: IoU 3/11 and 5/10 - no PQ match
    check(ev.instance_metrics_of([10], [4, 5], [[0, 0, 3], [1, 0, 5]]), n_inst_ref=1, n_inst_pred=2, inst_TP=1, inst_FN=0, inst_FP=0,
          inst_recall=1.0, inst_precision=1.0, inst_F1=1.0, FN_inst_vox=0, FP_inst_vox=0, PQ=0.0, SQ=0.0, RQ=0.0)


def test_two_lesions_bridged_by_one_predicted_blob():
    # R = 6 and 4 voxels, P = 12 voxels holding both: IoU 6/12 and 4/12
    check(ev.instance_metrics_of([6, 4], [12], [[0, 0, 6], [0, 1, 4]]), n_inst_ref=2, n_inst_pred=1, inst_TP=2, inst_FN=0, inst_FP=0,
          inst_recall=1.0, inst_precision=1.0, inst_F1=1.0, PQ=0.0, SQ=0.0, RQ=0.0)


def test_a_pure_false_positive_and_a_pure_miss():
    # R_0 matched by P_0 with IoU 8/10; R_1 (7 voxels) missed; P_1 (3 voxels) touches nothing
    got = ev.instance_metrics_of([9, 7], [9, 3], [[0, 0, 8]])
    rq = 1 / (1 + 0.5 + 0.5)
    check(got, n_inst_ref=2, n_inst_pred=2, inst_TP=1, inst_FN=1, inst_FP=1, inst_recall=0.5, inst_precision=0.5, inst_F1=0.5,
          FN_inst_vox=7, FP_inst_vox=3, SQ=0.8, RQ=rq, PQ=0.8 * rq)


def test_iou_of_exactly_one_half_is_no_match():
    check(ev.instance_metrics_of([3], [3], [[0, 0, 2]]), inst_TP=1, PQ=0.0, SQ=0.0, RQ=0.0)             # 2 / (3 + 3 - 2)
    check(ev.instance_metrics_of([2 ** 31 - 1], [2 ** 31 - 1], [[0, 0, (2 ** 32 - 2) // 3 + 1]]), RQ=1.0)   # just above
    check(ev.instance_metrics_of([4], [5], [[0, 0, 3]]), PQ=0.0, SQ=0.0, RQ=0.0)                         # 3 / 6
    check(ev.instance_metrics_of([4], [4], [[0, 0, 3]]), SQ=0.6, RQ=1.0, PQ=0.6)                         # 3 / 5


def test_every_empty_side():
    none = np.zeros((0, 3), np.int64)
    check(ev.instance_metrics_of([], [], none), n_inst_ref=0, n_inst_pred=0, inst_TP=0, inst_FN=0, inst_FP=0, inst_recall=NAN,
          inst_precision=NAN, inst_F1=NAN, FN_inst_vox=0, FP_inst_vox=0, PQ=NAN, SQ=NAN, RQ=NAN)
    check(ev.instance_metrics_of([5, 2], [], none), n_inst_ref=2, n_inst_pred=0, inst_TP=0, inst_FN=2, inst_FP=0, inst_recall=0.0,
          inst_precision=NAN, inst_F1=NAN, FN_inst_vox=7, FP_inst_vox=0, PQ=0.0, SQ=0.0, RQ=0.0)
    check(ev.instance_metrics_of([], [5, 2, 1], none), n_inst_ref=0, n_inst_pred=3, inst_TP=0, inst_FN=0, inst_FP=3, inst_recall=NAN,
          inst_precision=0.0, inst_F1=NAN, FN_inst_vox=0, FP_inst_vox=8, PQ=0.0, SQ=0.0, RQ=0.0)


def test_f1_is_zero_when_both_sides_exist_and_nothing_meets():
    check(ev.instance_metrics_of([5], [4], np.zeros((0, 3), np.int64)), inst_recall=0.0, inst_precision=0.0, inst_F1=0.0, inst_FN=1,
          inst_FP=1, FN_inst_vox=5, FP_inst_vox=4, PQ=0.0, SQ=0.0, RQ=0.0)


# ---- against the yardstick on small maps
sparse_pair = ir.sparse_pair

SMALL = [((9, 17, 35), 1), ((6, 6, 6), 2), ((1, 40, 70), 3), ((3, 3, 3), 4), ((1, 1, 1), 5)]


@pytest.mark.parametrize('shape,seed', SMALL)
def test_metrics_match_the_yardstick_on_small_maps(shape, seed):
    ref, pred = sparse_pair(shape, seed, density=0.08)
    for r in (1, 2, 3, (1, 2), (1, 2, 3)):
        lists = ir.overlaps(ref, pred, r)
        got, want = ev.instance_metrics_of(lists['ref_sizes'], lists['pred_sizes'], lists['pairs']), ir.metrics(
            lists['ref_sizes'], lists['pred_sizes'], lists['pairs'])
        check(got, **want)


@pytest.mark.parametrize('shape,seed', SMALL)
def test_the_records_merge_into_the_yardsticks_lists(shape, seed):
    ref, pred = sparse_pair(shape, seed, density=0.08)
    regions = [3, (1, 2)]
    n_out, rec = ir.records(ref, pred, regions)
    got = ev.overlaps_from_records(n_out, rec, len(regions))
    for g, r in enumerate(regions):
        want = ir.overlaps(ref, pred, r)
        for k in ('ref_sizes', 'pred_sizes', 'pairs'):
            assert got[g][k].dtype == np.int64 and np.array_equal(got[g][k], want[k]), (r, k)
        assert got[g]['pairs'].shape[1] == 3


def test_a_ring_against_two_arcs_has_several_pieces_per_pair():
    ref, pred = ir.ring_and_arcs()
    n_out, rec = ir.records(ref, pred, [1])
    assert list(n_out) == [1, 2, 4]
    got = ev.overlaps_from_records(n_out, rec, 1)[0]
    assert got['pairs'].tolist() == [[0, 0, 6], [1, 0, 6]]
    assert got['ref_sizes'].tolist() == [24] and got['pred_sizes'].tolist() == [9, 9]


# ---- the plan of the calls
def test_overlapping_regions_are_split_into_calls_of_disjoint_sets():
    assert ev.plan_instance_calls([(1, 2, 3), (2, 3), 3]) == [[0], [1], [2]]
    assert ev.plan_instance_calls(list(range(1, 34))) == [list(range(33))]
    assert ev.plan_instance_calls([1, (1, 2), 2, 3, (3, 4)]) == [[0, 2, 3], [1, 4]]
    assert ev.plan_instance_calls([(1, 2), (3,), 4, (4, 1)]) == [[0, 1, 2], [3]]
    many = ev.plan_instance_calls(list(range(1, 1030)))
    assert [len(c) for c in many] == [1024, 5]
    with pytest.raises(ValueError, match='outside 0..65535'):
        ev.plan_instance_calls([70000])


# ---- the flag through compute_metrics, both device halves replaced by numpy
def numpy_counts(seg_ref, seg_preds, values, ignore_label=None, checked=False):
    out = []
    for p in seg_preds:
        cls = lambda a: np.searchsorted(values, a.reshape(-1)) * np.isin(a.reshape(-1), values) + len(values) * ~np.isin(a.reshape(-1), values)
        m = np.zeros((len(values) + 1,) * 2, np.int64)
        np.add.at(m, (cls(np.asarray(seg_ref)), cls(np.asarray(p))), 1)
        out.append(m)
    return np.stack(out)


@pytest.fixture
def host_halves(monkeypatch):
    """evaluation's two device calls answered by numpy and the yardstick's records; returns the list of instance calls made."""
    made = []

    def overlaps(seg_ref, seg_pred, labels_or_regions, checked=False, **kw):
        made.append(list(labels_or_regions))
        out = {}
        for idx in ev.plan_instance_calls(labels_or_regions):
            regions = [labels_or_regions[k] for k in idx]
            n_out, rec = ir.records(np.asarray(seg_ref), np.asarray(seg_pred), regions)
            out.update(zip(regions, ev.overlaps_from_records(n_out, rec, len(regions))))
        return out

    monkeypatch.setattr(ev, 'confusion_counts', numpy_counts)
    monkeypatch.setattr(ev, 'instance_overlaps', overlaps)
    return made


def test_flag_off_keeps_the_eight_keys_and_makes_no_instance_call(host_halves):
    ref, pred = sparse_pair((6, 7, 8), 11, density=0.1)
    regions = [1, (2, 3)]
    off = ev.compute_metrics(ref, pred, regions)['metrics']
    assert [list(off[r]) for r in regions] == [EIGHT, EIGHT] and host_halves == []
    summary = ev.compute_metrics_on_arrays([ref], [pred], regions)
    assert sorted(summary['mean'][1]) == sorted(EIGHT) and host_halves == []
    on = ev.compute_metrics(ref, pred, regions, instance_metrics=True)['metrics']
    want = ir.case_metrics(ref, pred, regions)
    for r in regions:
        assert list(on[r]) == EIGHT + list(ev.INSTANCE_KEYS)
        assert all(ir.same_value(on[r][k], off[r][k]) for k in EIGHT)
        check({k: on[r][k] for k in ev.INSTANCE_KEYS}, **want[r])
    assert host_halves == [regions]


def test_an_ignore_label_is_refused_before_any_gpu_call(monkeypatch):
    def boom(*a, **k):
        raise AssertionError('a device call was made')
    for name in ('confusion_counts', 'instance_overlaps', 'surface_count', 'surface_distances', 'decode_labels'):
        monkeypatch.setattr(capi, name, boom)
    monkeypatch.setattr(capi, 'load_library', boom)
    seg = np.zeros((2, 2, 2), np.uint8)
    with pytest.raises(ValueError, match='instance metrics are refused together with an ignore label'):
        ev.compute_metrics(seg, seg, [1], ignore_label=2, instance_metrics=True)
    with pytest.raises(ValueError, match='instance metrics are refused together with an ignore label'):
        ev.compute_metrics_on_arrays([seg], [seg], [1], ignore_label=2, instance_metrics=True)
    with pytest.raises(ValueError, match='instance metrics are refused together with an ignore label'):
        ev.compute_metrics_on_files(['a.nii.gz'], ['b.nii.gz'], None, [1], ignore_label=2, instance_metrics=True)


def test_the_keys_ride_through_aggregate_and_summary_json(host_halves, tmp_path):
    pairs = [sparse_pair((6, 7, 8), 20 + k, density=0.1) for k in range(3)]
    pairs[1][0][pairs[1][0] == 2] = 0
    pairs[1][1][pairs[1][1] == 2] = 0                                   # label 2 absent on both sides of case 1
    regions = [1, 2, (1, 2, 3)]
    out = os.path.join(tmp_path, 'summary.json')
    summary = ev.compute_metrics_on_arrays([p[0] for p in pairs], [p[1] for p in pairs], regions, output_file=out,
                                           instance_metrics=True)
    wants = [ir.case_metrics(r, p, regions) for r, p in pairs]
    assert math.isnan(float(wants[1][2]['inst_F1'])) and math.isnan(float(wants[1][2]['PQ']))
    loaded = ev.load_summary_json(out)
    for got in (summary, loaded):
        for r in regions:
            for k in ev.INSTANCE_KEYS:
                vals = [float(w[r][k]) for w in wants]
                mean = NAN if all(math.isnan(v) for v in vals) else float(np.nanmean(vals))
                assert ir.same_value(got['mean'][r][k], mean), (r, k)
                assert all(ir.same_value(c['metrics'][r][k], v) for c, v in zip(got['metric_per_case'], vals))
        assert set(ev.INSTANCE_KEYS) <= set(got['foreground_mean'])
    assert list(summary['metric_per_case'][0]['metrics'][1]) == EIGHT + list(ev.INSTANCE_KEYS)
    assert type(summary['metric_per_case'][0]['metrics'][1]['n_inst_ref']) is int
