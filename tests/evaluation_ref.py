"""Host restatements shared by tests/test_evaluation_cpu.py and tests/test_gpu_evaluation.py: confusion matrices by
``np.bincount``, the golden data of tests/golden/make_golden_evaluation.py, and a host backend for the postprocessing
search (the scipy restatement of the labelling, bincount for the counts)."""
import contextlib
import json
import os

import numpy as np

from test_postprocessing_cpu import apply_ref, keep_largest_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def bincount_matrix(ref, pred, values, ignore=None):
    """int64 [C+1, C+1] of (reference class, predicted class); class C is every value not in ``values``."""
    values = list(values)
    cls = np.full(65536, len(values), np.int64)
    cls[values] = np.arange(len(values))
    ref = np.asarray(ref).reshape(-1).astype(np.int64)
    pred = np.asarray(pred).reshape(-1).astype(np.int64)
    if ignore is not None:
        keep = ref != ignore
        ref, pred = ref[keep], pred[keep]
    c = len(values) + 1
    return np.bincount(cls[ref] * c + cls[pred], minlength=c * c).reshape(c, c)


class HostBackend:
    def context(self):
        return contextlib.nullcontext()

    def put(self, seg):
        return np.array(seg, copy=True)

    def keep_largest(self, seg, sets):
        for s in sets:                      # disjoint sets, background 0 in none of them: one at a time is the same
            seg = keep_largest_ref(seg, [tuple(sorted(s))], 0)
        return seg

    def counts(self, ref, maps, values, ignore):
        return np.stack([bincount_matrix(ref, m, values, ignore) for m in maps])

    def host(self, seg):
        return seg

    def apply(self, seg, pp_fns, pp_fn_kwargs):
        return apply_ref(seg, pp_fn_kwargs)


def untyped(v):
    """Inverse of make_golden_evaluation.typed: (value, type description)."""
    if isinstance(v, dict):
        return {untyped(k)[0]: untyped(x)[0] for k, x in v['__dict__']}, \
            [(untyped(k)[1], untyped(x)[1]) for k, x in v['__dict__']]
    t, val = v
    if t in ('list', 'tuple'):
        items = [untyped(x) for x in val]
        seq = [i[0] for i in items]
        return (tuple(seq) if t == 'tuple' else seq), (t, [i[1] for i in items])
    return val, t


def type_tree(v):
    """The same type description for a live value."""
    if isinstance(v, dict):
        return [(type_tree(k), type_tree(x)) for k, x in v.items()]
    if isinstance(v, (list, tuple)):
        return (type(v).__name__, [type_tree(x) for x in v])
    return type(v).__name__


def load_golden():
    with open(os.path.join(GOLDEN, 'evaluation.json')) as f:
        meta = json.load(f)
    arrays = np.load(os.path.join(GOLDEN, 'evaluation.npz'), allow_pickle=False)
    return meta, arrays


def dataset_maps(meta, arrays, name):
    names = meta[name]['names']
    refs = [arrays[f'{name}__{n}__ref'] for n in names]
    preds = [arrays[f'{name}__{n}__pred'] for n in names]
    return names, refs, preds


def same(a, b):
    """Equality with NaN == NaN, for nested summaries."""
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return isinstance(b, (list, tuple)) and len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if isinstance(a, float) and isinstance(b, float) and np.isnan(a) and np.isnan(b):
        return True
    return a == b and type(a) is type(b)
