"""Evaluation and the postprocessing search on one MI355X: fnn_confusion_counts against np.bincount, the device metrics
and determine_postprocessing against the golden data made by the reference (tests/golden/make_golden_evaluation.py),
and the fused per-label search against a sequential one."""
import json
import os

import numpy as np
import pytest
import torch

from evaluation_ref import bincount_matrix, dataset_maps, load_golden, same, type_tree, untyped
from test_postprocessing_cpu import keep_largest_ref

pytestmark = pytest.mark.gpu

META, ARRAYS = load_golden()
DATASETS = sorted(META)


def _counts(ref, preds, values, ignore=None):
    from fast_nnunet_amd import evaluation as ev
    return ev.confusion_counts(ref, preds, values, ignore)


def _check(ref, preds, values, ignore=None):
    got = _counts(ref, preds, values, ignore)
    assert got.dtype == np.int64 and got.shape == (len(preds), len(values) + 1, len(values) + 1)
    for p, g in zip(preds, got):
        want = bincount_matrix(ref, p, values, ignore)
        assert np.array_equal(g, want), np.argwhere(g != want)[:5]


def _blocky(rng, n, hi, dtype, block=8):
    small = rng.integers(0, hi + 1, (max(1, n // block) + 1,))
    out = np.repeat(small, block)[:n].astype(dtype)
    noise = rng.random(n) < 0.05
    out[noise] = rng.integers(0, hi + 1, int(noise.sum()))
    return out


@pytest.mark.parametrize('seed', range(12))
def test_counts_equal_bincount(seed):
    rng = np.random.default_rng(4000 + seed)
    u16 = seed % 2 == 1
    n_classes = [2, 5, 17, 61, 118, 255][seed % 6]
    hi = 300 if u16 else 255
    values = sorted(rng.choice(np.arange(1, hi), n_classes, replace=False).tolist())
    n = int(rng.integers(1, 200000))
    ref = _blocky(rng, n, hi, np.uint16 if u16 else np.uint8)
    n_pred = 1 + seed % 4
    preds = [np.where(rng.random(n) < 0.2, _blocky(rng, n, hi, ref.dtype), ref).astype(ref.dtype) for _ in range(n_pred)]
    ignore = None if seed % 3 == 0 else int(ref[0])
    if ignore is not None and ignore in values:
        values.remove(ignore)
    _check(ref, preds, values, ignore)


def test_counts_edge_sizes_and_background():
    rng = np.random.default_rng(5)
    for n in (0, 1, 15, 16, 17, 8191, 8192 * 512 + 3):
        ref = rng.integers(0, 4, n).astype(np.uint8)
        pred = rng.integers(0, 4, n).astype(np.uint8)
        _check(ref, [pred, ref], [1, 2])
    bg = np.zeros(100003, np.uint8)
    got = _counts(bg, [bg, bg], [1, 2, 3])
    assert got[:, 3, 3].tolist() == [100003, 100003] and got.sum() == 2 * 100003
    got = _counts(bg, [bg], [1], ignore=0)
    assert got.sum() == 0


def test_counts_row_bands_and_many_predictions():
    rng = np.random.default_rng(6)
    n = 300001
    ref = rng.integers(0, 256, n).astype(np.uint8)
    preds = [rng.integers(0, 256, n).astype(np.uint8) for _ in range(6)]       # two passes: 4 + 2 predictions
    values = list(range(1, 256))                                               # 256 x 256 bins: bands of rows
    _check(ref, preds, [v for v in values if v != 7], ignore=7)
    vals2 = list(range(0, 256, 2))
    _check(ref.astype(np.uint16) * 200, [p.astype(np.uint16) * 200 for p in preds[:3]], [v * 200 for v in vals2[:100]])


def test_counts_from_device_tensors_and_dtypes():
    rng = np.random.default_rng(7)
    ref = rng.integers(0, 6, (33, 17, 9)).astype(np.int64)
    pred = rng.integers(0, 6, (33, 17, 9)).astype(np.int32)
    dev = torch.device('cuda', 0)
    t_ref, t_pred = torch.from_numpy(ref).to(dev), torch.from_numpy(pred).to(dev)
    got = _counts(t_ref, [t_pred], [1, 2, 3], ignore=5)
    assert np.array_equal(got[0], bincount_matrix(ref, pred, [1, 2, 3], 5))
    assert torch.equal(t_ref.cpu(), torch.from_numpy(ref)) and torch.equal(t_pred.cpu(), torch.from_numpy(pred))
    u8 = torch.from_numpy(ref.astype(np.uint8)).to(dev)[:, 1:]                  # a strided view
    got = _counts(u8, [u8.clone()], [1, 2])
    assert np.array_equal(got[0], bincount_matrix(ref[:, 1:], ref[:, 1:], [1, 2]))


def test_counts_512_cubed_61_classes():
    from tools.postprocess_bench import make_map
    seg = make_map(512)
    rng = np.random.default_rng(9)
    pred = seg.copy()
    idx = rng.integers(0, pred.size, 2_000_000)
    pred.reshape(-1)[idx] = rng.integers(0, 61, idx.size).astype(np.uint8)
    _check(seg, [pred], list(range(1, 61)))


@pytest.mark.parametrize('name', DATASETS)
@pytest.mark.parametrize('on_device', [False, True])
def test_device_metrics_equal_golden(name, on_device, tmp_path):
    from fast_nnunet_amd import evaluation as ev
    from fast_nnunet_amd.plans import LabelManager
    names, refs, preds = dataset_maps(META, ARRAYS, name)
    dj = META[name]['dataset_json']
    lm = LabelManager(dj['labels'], dj.get('regions_class_order'))
    lor = list(lm.foreground_regions) if lm.has_regions else [np.int64(v) for v in lm.foreground_labels]
    if on_device:
        refs = [torch.from_numpy(r).cuda() for r in refs]
        preds = [torch.from_numpy(p[None]).cuda() for p in preds]       # [1, X, Y, Z] as the reference reads them
        refs = [r[None] for r in refs]
    for r, p, golden in zip(refs, preds, META[name]['per_case_metrics']):
        res = ev.compute_metrics(r, p, lor, lm.ignore_label)
        want, want_types = untyped(golden)
        assert type_tree(res['metrics']) == want_types
        assert same(ev.json_ready(res['metrics']), want)
    out = os.path.join(tmp_path, 'summary.json')
    summary = ev.compute_metrics_on_arrays(refs, preds, lor, lm.ignore_label, names=names, output_file=out)
    with open(out) as f:
        mine = json.load(f)
    want = json.loads(json.dumps(META[name]['baseline_summary']))
    for case in want['metric_per_case']:
        case['reference_file'] = case['prediction_file'] = None
    for case in mine['metric_per_case']:
        case['reference_file'] = case['prediction_file'] = None
    assert same(mine, want)
    assert same(ev.load_summary_json(out)['mean'], summary['mean'])


@pytest.mark.parametrize('name', DATASETS)
def test_device_determine_postprocessing_equals_golden(name, tmp_path):
    from fast_nnunet_amd import postprocessing as pp
    names, refs, preds = dataset_maps(META, ARRAYS, name)
    before = [p.copy() for p in preds] + [r.copy() for r in refs]
    fns, kwargs = pp.determine_postprocessing(dict(zip(names, preds)), dict(zip(names, refs)), META[name]['dataset_json'],
                                              output_folder=str(tmp_path), save_postprocessed=True)
    assert all(np.array_equal(a, b) for a, b in zip(preds + refs, before))
    want, want_types = untyped(META[name]['kwargs'])
    assert kwargs == want and type_tree(kwargs) == want_types
    with open(os.path.join(tmp_path, 'postprocessing.json')) as f:
        assert same(json.load(f), META[name]['postprocessing_json'])
    with open(os.path.join(tmp_path, 'postprocessed', 'summary.json')) as f:
        final = json.load(f)
    assert same(final['mean'], META[name]['final_summary']['mean'])
    for n in names:
        assert np.array_equal(np.load(os.path.join(tmp_path, 'postprocessed', n + '.npy')),
                              ARRAYS[f'{name}__{n}__postprocessed'])
    fns2, kws2 = pp.load_postprocessing_pkl(os.path.join(tmp_path, 'postprocessing.pkl'))
    pkl_want, pkl_types = untyped(META[name]['pkl_kwargs'])
    assert kws2 == pkl_want and type_tree(kws2) == pkl_types


def _sequential_search(preds, refs, labels):
    """The reference's loop as written, on the host: whole foreground, then one labelling per label on the current
    source of every case.  Returns (kwargs, final per-class mean Dice)."""
    from fast_nnunet_amd import evaluation as ev

    def summary(maps):
        ms = [ev.metrics_from_counts(bincount_matrix(r, m, labels), labels) for r, m in zip(refs, maps)]
        return ev.aggregate([ev.case_result(m) for m in ms], labels)

    base = summary(preds)
    fg = [keep_largest_ref(p, labels) for p in preds]
    fg_sum = summary(fg)
    kwargs, source, cur = [], preds, base
    ok = fg_sum['foreground_mean']['Dice'] > base['foreground_mean']['Dice'] and \
        not any(fg_sum['mean'][k]['Dice'] < base['mean'][k]['Dice'] for k in fg_sum['mean'])
    if ok:
        kwargs.append({'labels_or_regions': [int(v) for v in labels]})
        source, cur = fg, fg_sum
    for l in labels:
        cand = [keep_largest_ref(s, l) for s in source]
        cand_sum = summary(cand)
        if cand_sum['mean'][l]['Dice'] > cur['mean'][l]['Dice']:
            kwargs.append({'labels_or_regions': int(l)})
            source, cur = cand, cand_sum
    return kwargs, cur


def _random_cases(rng, n_cases, n_labels=61):
    """48 x 48 x 40 maps: each label a box in a cell of its own, some with a true second blob, predictions with
    islands of random labels in the gaps - per-label steps accepted, rejected and tied."""
    preds, refs = [], []
    for _ in range(n_cases):
        ref = np.zeros((48, 48, 40), np.uint8)
        cells = rng.permutation(64)[:n_labels]
        for lab, c in enumerate(cells, start=1):
            x, y, z = (c // 16) * 12, ((c // 4) % 4) * 12, (c % 4) * 10
            ref[x + 1:x + 10, y + 1:y + 10, z + 1:z + 8] = lab
            if lab % 5 == 0:
                ref[x + 11, y + 11, z + 9] = lab                   # a true second component
        pred = ref.copy()
        pred[ref > 0] = np.where(rng.random(int((ref > 0).sum())) < 0.02, 0, ref[ref > 0])
        gaps = np.flatnonzero(ref == 0)
        idx = rng.choice(gaps, 150, replace=False)
        pred.reshape(-1)[idx] = rng.integers(1, n_labels // 2, idx.size).astype(np.uint8)
        refs.append(ref)
        preds.append(pred)
    return preds, refs


def test_fused_search_equals_sequential_on_61_labels(tmp_path):
    from fast_nnunet_amd import postprocessing as pp
    rng = np.random.default_rng(61)
    preds, refs = _random_cases(rng, 3)
    dj = {'labels': {'background': 0, **{f'l{i}': i for i in range(1, 62)}}}
    before = [p.copy() for p in preds] + [r.copy() for r in refs]
    fns, kwargs = pp.determine_postprocessing(preds, refs, dj, output_folder=str(tmp_path))
    assert all(np.array_equal(a, b) for a, b in zip(preds + refs, before))
    want_kwargs, want_final = _sequential_search(preds, refs, [np.int64(i) for i in range(1, 62)])
    assert kwargs == want_kwargs and len(kwargs) > 1
    with open(os.path.join(tmp_path, 'postprocessed', 'summary.json')) as f:
        final = json.load(f)
    assert same(final['foreground_mean'], want_final['foreground_mean'])
    assert same(final['mean'], {str(k): v for k, v in want_final['mean'].items()})
