"""Evaluation and the postprocessing search without a GPU: the host half of fast_nnunet_amd.evaluation and the
decisions of determine_postprocessing, checked against golden data made by the reference itself
(tests/golden/make_golden_evaluation.py)."""
import json
import os
import pickle
import sys
import types

import numpy as np
import pytest

from evaluation_ref import HostBackend, bincount_matrix, dataset_maps, load_golden, same, type_tree, untyped

META, ARRAYS = load_golden()
DATASETS = sorted(META)


def _lm(name):
    from fast_nnunet_amd.plans import LabelManager
    dj = META[name]['dataset_json']
    return LabelManager(dj['labels'], dj.get('regions_class_order'))


def _labels_or_regions(name):
    lm = _lm(name)
    return list(lm.foreground_regions) if lm.has_regions else [np.int64(v) for v in lm.foreground_labels]


def _host_results(name):
    from fast_nnunet_amd import evaluation as ev
    names, refs, preds = dataset_maps(META, ARRAYS, name)
    lor = _labels_or_regions(name)
    values = ev.count_classes(lor)
    ignore = _lm(name).ignore_label
    return [ev.metrics_from_counts(bincount_matrix(r, p, values, ignore), lor) for r, p in zip(refs, preds)], names, lor


def _json(path):
    with open(path) as f:
        return json.load(f)


def test_golden_covers_every_decision_kind():
    kinds = {n: META[n]['postprocessing_json']['postprocessing_kwargs'] for n in DATASETS}
    assert kinds['labels_mixed'] == [{'labels_or_regions': [1, 2, 3]}, {'labels_or_regions': 1}]
    assert kinds['labels_fg_rejected'] == [{'labels_or_regions': 1}]
    assert np.isnan(META['absent']['baseline_summary']['foreground_mean']['Dice'])
    assert any(len(k['labels_or_regions']) > 1 for k in kinds['regions'][1:] if isinstance(k['labels_or_regions'], list))
    # labels_fg_rejected: the whole-foreground step raises foreground_mean, but class 2 falls
    from fast_nnunet_amd import evaluation as ev
    from test_postprocessing_cpu import keep_largest_ref
    _, refs, preds = dataset_maps(META, ARRAYS, 'labels_fg_rejected')
    lor = _labels_or_regions('labels_fg_rejected')

    def summary(maps):
        return ev.aggregate([ev.case_result(ev.metrics_from_counts(bincount_matrix(r, m, [1, 2]), lor))
                             for r, m in zip(refs, maps)], lor)
    base, fg = summary(preds), summary([keep_largest_ref(p, [1, 2]) for p in preds])
    assert fg['foreground_mean']['Dice'] > base['foreground_mean']['Dice']
    assert fg['mean'][2]['Dice'] < base['mean'][2]['Dice']
    # labels_mixed: label 3 ties its baseline and is rejected
    pj = META['labels_mixed']['postprocessing_json']
    assert pj['postprocessed']['mean']['3']['Dice'] == 1.0 and {'labels_or_regions': 3} not in kinds['labels_mixed']


@pytest.mark.parametrize('name', DATASETS)
def test_metrics_from_counts_equal_reference_per_case(name):
    from fast_nnunet_amd import evaluation as ev
    got, _, _ = _host_results(name)
    assert len(got) == len(META[name]['per_case_metrics'])
    for mine, golden in zip(got, META[name]['per_case_metrics']):
        want, want_types = untyped(golden)
        assert type_tree(mine) == want_types               # numpy scalar types, and float NaN where the reference has it
        assert same(ev.json_ready(mine), want)             # values, bit for bit


@pytest.mark.parametrize('name', DATASETS)
def test_aggregation_equals_reference_summary(name, tmp_path):
    from fast_nnunet_amd import evaluation as ev
    got, names, lor = _host_results(name)
    summary = ev.aggregate([ev.case_result(m, n, n) for m, n in zip(got, names)], lor)
    path = os.path.join(tmp_path, 'summary.json')
    ev.save_summary_json(summary, path)
    want = META[name]['baseline_summary']
    mine = _json(path)
    for case in want['metric_per_case']:                   # the reference names files; these are arrays
        case['reference_file'] = case['prediction_file'] = None
    for case in mine['metric_per_case']:
        case['reference_file'] = case['prediction_file'] = None
    assert same(mine, want)
    back = ev.load_summary_json(path)
    assert same(back['mean'], summary['mean']) and same(back['foreground_mean'], summary['foreground_mean'])
    assert same(back['metric_per_case'][0]['metrics'], summary['metric_per_case'][0]['metrics'])
    assert list(back['mean'].keys()) == list(summary['mean'].keys())


@pytest.mark.parametrize('name', DATASETS)
def test_decisions_equal_reference(name, tmp_path):
    from fast_nnunet_amd import postprocessing as pp
    names, refs, preds = dataset_maps(META, ARRAYS, name)
    before = [p.copy() for p in preds]
    fns, kwargs = pp.determine_postprocessing(dict(zip(names, preds)), dict(zip(names, refs)),
                                              META[name]['dataset_json'], output_folder=str(tmp_path),
                                              save_postprocessed=True, backend=HostBackend())
    assert all(np.array_equal(a, b) for a, b in zip(preds, before))
    want, want_types = untyped(META[name]['kwargs'])
    assert kwargs == want and type_tree(kwargs) == want_types
    assert fns == [pp.remove_all_but_largest_component_from_segmentation] * len(want)
    assert same(_json(os.path.join(tmp_path, 'postprocessing.json')), META[name]['postprocessing_json'])
    final = _json(os.path.join(tmp_path, 'postprocessed', 'summary.json'))
    golden_final = META[name]['final_summary']
    assert same(final['mean'], golden_final['mean']) and same(final['foreground_mean'], golden_final['foreground_mean'])
    for n in names:
        assert np.array_equal(np.load(os.path.join(tmp_path, 'postprocessed', n + '.npy')),
                              ARRAYS[f'{name}__{n}__postprocessed'])
    # the pkl: the reference's global, the reference's (numpy) kwarg types
    pkl = os.path.join(tmp_path, 'postprocessing.pkl')
    fns2, kws2 = pp.load_postprocessing_pkl(pkl)
    assert fns2 == fns
    pkl_want, pkl_types = untyped(META[name]['pkl_kwargs'])
    assert kws2 == pkl_want and type_tree(kws2) == pkl_types


def test_pkl_loads_under_the_reference_name(tmp_path):
    from fast_nnunet_amd import postprocessing as pp
    from fast_nnunet_amd.postprocessing_search import save_postprocessing_pkl
    mod_name, fn_name = pp.REFERENCE_NAME
    path = os.path.join(tmp_path, 'postprocessing.pkl')
    kwargs = [{'labels_or_regions': [np.int64(1), np.int64(2)]}, {'labels_or_regions': (2, 3)}]
    save_postprocessing_pkl([pp.remove_all_but_largest_component_from_segmentation] * 2, kwargs, path)
    names = ['nnunetv2', 'nnunetv2.postprocessing', mod_name]
    saved = {n: sys.modules.get(n) for n in names}
    try:
        for n in names:
            sys.modules[n] = types.ModuleType(n)

        def stand_in(segmentation, labels_or_regions, background_label=0):
            raise AssertionError('never called')
        setattr(sys.modules[mod_name], fn_name, stand_in)
        with open(path, 'rb') as f:
            fns, kws = pickle.load(f)
    finally:
        for n, m in saved.items():
            if m is None:
                sys.modules.pop(n, None)
            else:
                sys.modules[n] = m
    assert fns == [stand_in, stand_in]
    assert kws[0]['labels_or_regions'] == [1, 2] and type(kws[0]['labels_or_regions'][0]) is np.int64
    assert kws[1] == {'labels_or_regions': (2, 3)}


def test_json_ready_and_keys():
    from fast_nnunet_amd import evaluation as ev
    d = ev.json_ready({np.int64(3): {'a': np.float32(0.5), 'b': np.int32(2), 'c': np.bool_(True), 'd': float('nan'),
                                     'e': (np.uint8(1), np.int64(2)), 'f': np.arange(2)}})
    assert list(d) == [3] and type(list(d)[0]) is int
    v = d[3]
    assert v['a'] == 0.5 and type(v['a']) is float and type(v['b']) is int and v['c'] is True
    assert np.isnan(v['d']) and v['e'] == (1, 2) and type(v['e'][0]) is int and v['f'] == [0, 1]
    assert ev.key_to_label_or_region(ev.label_or_region_to_key((1, 2))) == (1, 2)
    assert ev.key_to_label_or_region(ev.label_or_region_to_key((3,))) == (3,)
    assert ev.key_to_label_or_region('7') == 7


def test_count_classes_and_table():
    from fast_nnunet_amd import evaluation as ev
    assert ev.count_classes([np.int64(3), (1, 2), 2]) == [1, 2, 3]
    assert ev.class_table([1, 4]).tolist() == [-1, 0, -1, -1, 1]
    with pytest.raises(ValueError):
        ev.count_classes(list(range(1, 300)))
    with pytest.raises(ValueError):
        ev.metrics_from_counts(np.zeros((3, 3), np.int64), [1, 2, 3])


def test_argument_checks():
    from fast_nnunet_amd import evaluation as ev
    a = np.zeros((4, 5, 6), np.uint8)
    with pytest.raises(ValueError, match='shape'):
        ev.compute_metrics(a, np.zeros((4, 5, 7), np.uint8), [1])
    with pytest.raises(ValueError, match='integer'):
        ev.compute_metrics(a, a.astype(np.float32), [1])
    with pytest.raises(ValueError, match='integer'):
        ev.compute_metrics(a, a.astype(bool), [1])
    with pytest.raises(ValueError, match='0..65535'):
        ev.compute_metrics(a, np.full(a.shape, 70000, np.int32), [1])
    with pytest.raises(ValueError, match='0..65535'):
        ev.compute_metrics(np.full(a.shape, -1, np.int16), a, [1])
    with pytest.raises(ValueError, match='ignore'):
        ev.compute_metrics(a, a, [1, 2], ignore_label=2)
    with pytest.raises(ValueError, match='json'):
        ev.compute_metrics_on_arrays([a], [a], [1], output_file='summary.txt')
    with pytest.raises(ValueError):
        ev.compute_metrics_on_arrays([a, a], [a], [1])


def test_search_pairs_by_name_and_warns(tmp_path):
    from fast_nnunet_amd import postprocessing as pp
    names, refs, preds = dataset_maps(META, ARRAYS, 'labels_mixed')
    with pytest.warns(UserWarning, match='Not all references'):
        fns, kws = pp.determine_postprocessing(dict(zip(names[:-1], preds[:-1])), dict(zip(names, refs)),
                                               META['labels_mixed']['dataset_json'], backend=HostBackend())
    with pytest.raises(ValueError, match='without a reference'):
        pp.determine_postprocessing({'x': preds[0]}, {'y': refs[0]}, META['labels_mixed']['dataset_json'],
                                    backend=HostBackend())
