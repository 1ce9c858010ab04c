#!/usr/bin/env python3
"""Generate ``evaluation.npz`` / ``evaluation.json`` FROM THE REFERENCE ITSELF (build container only: needs the
reference's sources).

    python tests/golden/make_golden_evaluation.py

Small seeded label datasets, each written as a folder of ``.npy`` predictions and references, are handed to the
reference's own ``compute_metrics``, ``compute_metrics_on_folder`` and ``determine_postprocessing``.  Stand-ins
installed here (not reference code): an ``.npy`` reader-writer under ``nnunetv2.imageio``, a serial pool in place of the
``spawn`` pool, and the scipy restatement of acvl_utils' ``remove_all_but_largest_component`` that
tests/test_postprocessing_cpu.py uses (full connectivity, every component of the largest size kept).

Stored: the maps (npz); per dataset the per-case compute_metrics dicts with their scalar types, the baseline and final
summaries, postprocessing.json, and the kwargs as returned and as pickled, with their types (json).
"""
from __future__ import annotations

import json
import os
import pickle
import sys
import tempfile
import types

import numpy as np
from scipy import ndimage

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import ref_shims  # noqa: E402

ref_shims.install()


def remove_all_but_largest_component(binary_image, connectivity=None):
    lab, n = ndimage.label(binary_image, structure=ndimage.generate_binary_structure(binary_image.ndim, binary_image.ndim))
    if n == 0:
        return np.zeros_like(binary_image, dtype=bool)
    sizes = np.bincount(lab.ravel())[1:]
    return np.isin(lab, np.flatnonzero(sizes == sizes.max()) + 1)


class NpyIO:
    def read_seg(self, fname):
        return np.load(fname)[None], {}

    def write_seg(self, seg, fname, properties):
        np.save(fname, seg)


class _SerialPool:
    def __init__(self, *a, **k):
        pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False

    def starmap(self, fn, args):
        return [fn(*a) for a in args]


_serial_mp = types.SimpleNamespace(get_context=lambda *_: types.SimpleNamespace(Pool=_SerialPool))

morph = types.ModuleType('acvl_utils.morphology.morphology_helper')
morph.remove_all_but_largest_component = remove_all_but_largest_component
sys.modules['acvl_utils.morphology.morphology_helper'] = morph
npy_mod = types.ModuleType('nnunetv2.imageio.npy_io')
npy_mod.NpyIO = NpyIO
sys.modules['nnunetv2.imageio.npy_io'] = npy_mod

import nnunetv2.evaluation.evaluate_predictions as ref_eval  # noqa: E402
import nnunetv2.postprocessing.remove_connected_components as ref_pp  # noqa: E402
from nnunetv2.utilities.plans_handling.plans_handler import PlansManager  # noqa: E402

ref_eval.multiprocessing = _serial_mp
ref_pp.multiprocessing = _serial_mp
PlansManager.image_reader_writer_class = property(lambda self: NpyIO)

PLANS = {'dataset_name': 'Dataset996_Eval', 'plans_name': 'nnUNetPlans', 'label_manager': 'LabelManager',
         'transpose_forward': [0, 1, 2], 'transpose_backward': [0, 1, 2], 'configurations': {}}


def _box(a, lo, hi, v):
    a[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = v


def _islands(rng, a, value, n, where=None):
    """n single voxels of ``value`` at random background positions (inside ``where`` if given)."""
    free = np.flatnonzero((a == 0) if where is None else where)
    a.reshape(-1)[rng.choice(free, n, replace=False)] = value


def labels_mixed(rng, shape):
    """fg step accepted; label 1 (islands) accepted, 2 (a true second blob) rejected, 3 (exact) a tie."""
    ref = np.zeros(shape, np.uint8)
    _box(ref, (4, 4, 4), (14, 16, 12), 1)
    _box(ref, (14, 4, 4), (18, 9, 12), 2)                  # blob A of 2, touching 1
    _box(ref, (4, 16, 4), (8, 19, 8), 2)                   # blob B of 2, touching 1, not A
    _box(ref, (8, 8, 12), (12, 12, 15), 3)                 # 3, touching 1
    pred = ref.copy()
    d = rng.integers(0, 2, 3)
    _box(pred, (4 + d[0], 4, 4), (14, 16 - d[1], 12), 1)   # slightly different extent of 1
    pred[(ref == 1) & (pred == 0)] = 0
    _islands(rng, pred, 1, int(rng.integers(3, 8)))
    far = np.zeros(shape, bool)
    _box(far, (0, 0, 0), (2, 2, 2), True)
    if rng.random() < 0.5:
        _islands(rng, pred, 2, 1, far & (pred == 0))       # a small spurious island of 2 in some cases
    return ref, pred


def labels_fg_rejected(rng, shape):
    """foreground_mean rises, but class 2 (a true blob away from the rest) gets worse: the fg step is rejected."""
    ref = np.zeros(shape, np.uint8)
    _box(ref, (3, 3, 3), (15, 15, 12), 1)
    _box(ref, (19, 18, 14), (20, 20, 16), 2)
    _box(ref, (15, 3, 3), (18, 10, 8), 2)
    pred = ref.copy()
    _islands(rng, pred, 1, int(rng.integers(500, 700)))
    return ref, pred


def ignore_case(rng, shape):
    """labels 1, 2 and the ignore label 3 in the reference; islands of 1 inside and outside ignored voxels."""
    ref = np.zeros(shape, np.uint8)
    _box(ref, (2, 2, 2), (12, 12, 10), 1)
    _box(ref, (12, 2, 2), (16, 8, 10), 2)
    _box(ref, (16, 12, 0), shape, 3)
    pred = np.where(ref == 3, 0, ref).astype(np.uint8)
    _islands(rng, pred, 1, 6, ref == 3)                    # not counted: under the ignore label
    _islands(rng, pred, 1, int(rng.integers(1, 4)), (ref == 0) & (pred == 0))
    _islands(rng, pred, 2, 2, (ref == 3) & (pred == 0))
    return ref, pred


def regions_case(rng, shape):
    """nested regions whole (1, 2, 3) > core (2, 3) > enhancing (3) with islands at each level."""
    ref = np.zeros(shape, np.uint8)
    _box(ref, (3, 3, 3), (17, 17, 14), 1)
    _box(ref, (6, 6, 5), (14, 14, 11), 2)
    _box(ref, (8, 8, 7), (12, 11, 9), 3)
    pred = ref.copy()
    _islands(rng, pred, 1, int(rng.integers(2, 6)))
    inside1 = pred == 1
    _islands(rng, pred, 2, int(rng.integers(1, 4)), inside1)
    _islands(rng, pred, 3, int(rng.integers(0, 3)) + 1, (pred == 1))
    if rng.random() < 0.5:
        _box(pred, (8, 8, 7), (9, 11, 9), 2)                # enhancing partly missed
    return ref, pred


def absent_case(rng, shape):
    """label 3 appears in no reference and no prediction: NaN Dice for it, foreground_mean NaN."""
    ref = np.zeros(shape, np.uint8)
    _box(ref, (2, 2, 2), (12, 14, 10), 1)
    _box(ref, (12, 2, 2), (15, 9, 6), 2)
    pred = ref.copy()
    _islands(rng, pred, 1, int(rng.integers(2, 6)))
    _islands(rng, pred, 2, int(rng.integers(0, 3)))
    return ref, pred


DATASETS = [
    dict(name='labels_mixed', labels={'background': 0, 'a': 1, 'b': 2, 'c': 3}, make=labels_mixed, cases=5,
         shape=(22, 24, 18), seed=1),
    dict(name='labels_fg_rejected', labels={'background': 0, 'a': 1, 'b': 2}, make=labels_fg_rejected, cases=4,
         shape=(24, 24, 20), seed=2),
    dict(name='ignore', labels={'background': 0, 'a': 1, 'b': 2, 'ignore': 3}, make=ignore_case, cases=4,
         shape=(20, 18, 14), seed=3),
    dict(name='regions', labels={'background': 0, 'whole': [1, 2, 3], 'core': [2, 3], 'enh': 3},
         regions_class_order=[1, 2, 3], make=regions_case, cases=5, shape=(20, 20, 16), seed=4),
    dict(name='absent', labels={'background': 0, 'a': 1, 'b': 2, 'c': 3}, make=absent_case, cases=4,
         shape=(18, 20, 14), seed=5),
]


def typed(v):
    """A JSON value that keeps the Python / numpy type name of every scalar: [type, value]."""
    if isinstance(v, dict):
        return {'__dict__': [[typed(k), typed(x)] for k, x in v.items()]}
    if isinstance(v, (list, tuple)):
        return [type(v).__name__, [typed(x) for x in v]]
    if isinstance(v, (np.generic, int, float, str, bool)) or v is None:
        val = v.item() if isinstance(v, np.generic) else v
        return [type(v).__name__, val]
    raise TypeError(type(v))


def main():
    arrays, meta = {}, {}
    for ds in DATASETS:
        rng = np.random.default_rng(900 + ds['seed'])
        dj = {'labels': ds['labels'], 'file_ending': '.npy'}
        if 'regions_class_order' in ds:
            dj['regions_class_order'] = ds['regions_class_order']
        lm = PlansManager(PLANS).get_label_manager(dj)
        lor = lm.foreground_regions if lm.has_regions else lm.foreground_labels
        with tempfile.TemporaryDirectory() as tmp:
            fp, fr = os.path.join(tmp, 'pred'), os.path.join(tmp, 'ref')
            os.makedirs(fp)
            os.makedirs(fr)
            names = []
            for c in range(ds['cases']):
                ref, pred = ds['make'](rng, ds['shape'])
                name = f'case_{c:03d}'
                names.append(name)
                np.save(os.path.join(fr, name + '.npy'), ref)
                np.save(os.path.join(fp, name + '.npy'), pred)
                arrays[f"{ds['name']}__{name}__ref"] = ref
                arrays[f"{ds['name']}__{name}__pred"] = pred
            per_case = [ref_eval.compute_metrics(os.path.join(fr, n + '.npy'), os.path.join(fp, n + '.npy'), NpyIO(),
                                                 lor, lm.ignore_label) for n in names]
            fns, kwargs = ref_pp.determine_postprocessing(fp, fr, PLANS, dj, num_processes=1)
            with open(os.path.join(fp, 'postprocessing.pkl'), 'rb') as f:
                _, pkl_kwargs = pickle.load(f)
            with open(os.path.join(fp, 'postprocessing.json')) as f:
                pp_json = json.load(f)
            with open(os.path.join(fp, 'summary.json')) as f:
                baseline = json.load(f)
            with open(os.path.join(fp, 'postprocessed', 'summary.json')) as f:
                final = json.load(f)
            for n in names:
                arrays[f"{ds['name']}__{n}__postprocessed"] = np.load(os.path.join(fp, 'postprocessed', n + '.npy'))
        meta[ds['name']] = {
            'dataset_json': dj, 'names': names,
            'per_case_metrics': [typed(r['metrics']) for r in per_case],
            'baseline_summary': baseline, 'final_summary': final, 'postprocessing_json': pp_json,
            'pp_fns': [f.__module__ + '.' + f.__name__ for f in fns],
            'kwargs': typed(kwargs), 'pkl_kwargs': typed(pkl_kwargs),
        }
        print(ds['name'], 'kwargs', kwargs, 'fg', baseline['foreground_mean']['Dice'])
    np.savez_compressed(os.path.join(HERE, 'evaluation.npz'), **arrays)
    with open(os.path.join(HERE, 'evaluation.json'), 'w') as f:
        json.dump(meta, f, indent=1)


if __name__ == '__main__':
    main()
