"""``determine_postprocessing`` on the GPU: which connected-component steps improve the Dice of a set of predictions.

Makes the decisions of nnunetv2's ``determine_postprocessing`` (postprocessing/remove_connected_components.py:52-245)
on label arrays in place of folders:

1. evaluate the predictions (the baseline);
2. try keeping the largest component of the whole foreground (``foreground_labels``, for region datasets too); accept it
   only if ``foreground_mean`` Dice rises strictly and no class's mean Dice falls;
3. with more than one label or region, try each in declaration order on the current source; accept a step if that
   class's mean Dice rises strictly.

Every comparison is made on the summary values the reference reads back from its summary.json files (float64, NaN
compares False).  Labelling is ``fnn_keep_largest_components``, counting ``fnn_confusion_counts``; the metrics are
computed on the host from the counts (``evaluation.metrics_from_counts``).  One case is on the device at a time.
"""
from __future__ import annotations

import os
import pickle
import types
import warnings
from typing import List, Mapping, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import evaluation as ev
from . import postprocessing as pp
from .plans import LabelManager


class _ReferencePickler(pickle._Pickler):
    """Writes this package's step function under the reference's global name, so nnU-Net itself loads the pkl."""
    dispatch = dict(pickle._Pickler.dispatch)

    def _save_function(self, obj, name=None):
        if obj is pp.remove_all_but_largest_component_from_segmentation and self.proto >= 4:
            self.save(pp.REFERENCE_NAME[0])
            self.save(pp.REFERENCE_NAME[1])
            self.write(pickle.STACK_GLOBAL)
            self.memoize(obj)
            return
        pickle._Pickler.save_global(self, obj, name)

    dispatch[types.FunctionType] = _save_function


def save_postprocessing_pkl(pp_fns, pp_fn_kwargs, path: str):
    """``postprocessing.pkl`` as the reference writes it (``save_pickle((pp_fns, pp_fn_kwargs))``)."""
    with open(path, 'wb') as f:
        _ReferencePickler(f, protocol=max(4, pickle.DEFAULT_PROTOCOL)).dump((list(pp_fns), list(pp_fn_kwargs)))


def _label_manager(dataset_json_or_label_manager) -> LabelManager:
    if isinstance(dataset_json_or_label_manager, dict):
        dj = dataset_json_or_label_manager
        return LabelManager(dj['labels'], dj.get('regions_class_order'))
    return dataset_json_or_label_manager


def _cases(predictions, references) -> List[Tuple[str, object, object]]:
    """(name, prediction, reference) in the order of the sorted prediction names; a sequence is named by position."""
    if not isinstance(predictions, Mapping):
        predictions = {f'case_{i:05d}': p for i, p in enumerate(predictions)}
    if not isinstance(references, Mapping):
        references = {f'case_{i:05d}': r for i, r in enumerate(references)}
    missing = [n for n in predictions if n not in references]
    if missing:
        raise ValueError(f'predictions without a reference: {missing[:5]}')
    if not all(n in predictions for n in references):
        warnings.warn('Not all references have a prediction. Determining postprocessing should always be done on the '
                      'entire dataset!')
    out = []
    for n in sorted(predictions):
        p, r = predictions[n], references[n]
        if ev._shape(p) != ev._shape(r):
            raise ValueError(f'{n}: shape mismatch: reference {ev._shape(r)}, prediction {ev._shape(p)}')
        if len(ev._shape(p)) not in (2, 3):
            raise ValueError(f'{n}: label maps must be 2-D or 3-D, got shape {ev._shape(p)}')
        ev.check_label_map(p)
        ev.check_label_map(r)
        out.append((n, p, r))
    return out


def _device_map(seg, dev: torch.device) -> torch.Tensor:
    """A device copy the labelling kernel can take (uint8 stays uint8, any other integer type becomes int32)."""
    if isinstance(seg, torch.Tensor):
        t = seg.to(dev)
        return t if t.dtype == torch.uint8 else t.to(torch.int32)
    arr = np.asarray(seg)
    return torch.from_numpy(np.ascontiguousarray(arr if arr.dtype == np.uint8 else arr.astype(np.int32))).to(dev)


def _host_copy(seg) -> np.ndarray:
    return seg.detach().cpu().numpy().copy() if isinstance(seg, torch.Tensor) else np.array(seg, copy=True)


def _summary(per_case: List[dict], names: List[str], labels_or_regions) -> dict:
    return ev.aggregate([ev.case_result(m, n, n) for m, n in zip(per_case, names)], labels_or_regions)


def _fg_improves(baseline: dict, candidate: dict) -> bool:
    do_this = candidate['foreground_mean']['Dice'] > baseline['foreground_mean']['Dice']
    if do_this:
        for k in candidate['mean'].keys():
            if candidate['mean'][k]['Dice'] < baseline['mean'][k]['Dice']:
                return False
    return do_this


def _class_mean_dice(per_case: List[dict], key) -> float:
    vals = [m[key]['Dice'] for m in per_case]
    if all(isinstance(v, float) and np.isnan(v) for v in vals):
        return float('nan')
    return float(np.nanmean(vals))


def _write_outputs(output_folder: str, baseline: dict, final: dict, pp_fns, pp_fn_kwargs):
    os.makedirs(os.path.join(output_folder, 'postprocessed'), exist_ok=True)
    ev.save_summary_json(baseline, os.path.join(output_folder, 'summary.json'))
    ev.save_summary_json(final, os.path.join(output_folder, 'postprocessed', 'summary.json'))
    save_postprocessing_pkl(pp_fns, pp_fn_kwargs, os.path.join(output_folder, 'postprocessing.pkl'))
    doc = {
        'input_folder': {'foreground_mean': baseline['foreground_mean'],
                         'mean': {ev.label_or_region_to_key(k): v for k, v in baseline['mean'].items()}},
        'postprocessed': {'foreground_mean': final['foreground_mean'],
                          'mean': {ev.label_or_region_to_key(k): v for k, v in final['mean'].items()}},
        'postprocessing_fns': [pp.REFERENCE_NAME[1] for _ in pp_fns],
        'postprocessing_kwargs': pp_fn_kwargs,
    }
    ev._dump_json(doc, os.path.join(output_folder, 'postprocessing.json'))


class DeviceBackend:
    """The GPU operations the search is made of: one case on the device at a time."""

    def __init__(self):
        self.dev = ev._device()

    def context(self):
        return torch.cuda.device(self.dev)

    def put(self, seg):
        return _device_map(seg, self.dev)

    def keep_largest(self, seg, sets: List[frozenset]):
        """Every set labelled in one pass (the sets are disjoint), background 0."""
        return pp._postprocess(seg, [sets], [0])

    def counts(self, ref, maps, values, ignore):
        return ev.confusion_counts(ref, maps, values, ignore, checked=True)

    def host(self, seg):
        return seg.cpu()

    def apply(self, seg, pp_fns, pp_fn_kwargs):
        return pp.apply_postprocessing(seg, pp_fns, pp_fn_kwargs)


def determine_postprocessing(predictions: Union[Sequence, Mapping[str, object]],
                             references: Union[Sequence, Mapping[str, object]],
                             dataset_json_or_label_manager, output_folder: Optional[str] = None,
                             save_postprocessed: bool = False, verbose: bool = False, backend=None):
    """The reference's ``determine_postprocessing`` on label maps (numpy or torch, 2-D or 3-D, values 0..65535).

    ``predictions`` / ``references``: sequences paired by position, or mappings paired by name (cases in the order of
    the sorted prediction names, as the reference lists its folder).  ``dataset_json_or_label_manager``: a
    ``dataset.json`` dict or a ``plans.LabelManager``.  Returns ``(pp_fns, pp_fn_kwargs)`` with this package's
    ``remove_all_but_largest_component_from_segmentation``.  With ``output_folder``, writes ``summary.json`` (baseline),
    ``postprocessed/summary.json`` (final), ``postprocessing.pkl`` (loadable by nnU-Net itself) and
    ``postprocessing.json``; with ``save_postprocessed`` also ``postprocessed/<name>.npy``.  The inputs are not
    modified.  ``backend``: the labelling and counting operations (default: the GPU, ``DeviceBackend``)."""
    lm = _label_manager(dataset_json_or_label_manager)
    fg_labels = [np.int64(v) for v in lm.foreground_labels]          # the reference's labels come from np.unique
    labels_or_regions = list(lm.foreground_regions) if lm.has_regions else list(fg_labels)
    if not labels_or_regions:
        raise ValueError('the dataset has no foreground label')
    ignore = lm.ignore_label
    ev._check_ignore(labels_or_regions, ignore)
    cases = _cases(predictions, references)
    if not cases:
        raise ValueError('no prediction to evaluate')
    be = backend if backend is not None else DeviceBackend()
    names = [n for n, _, _ in cases]
    values = ev.count_classes(labels_or_regions)
    fg_set = pp.label_set(list(fg_labels))
    per_step = len(labels_or_regions) > 1
    say = print if verbose else (lambda *a, **k: None)

    base_m, fg_m = [], []           # per case: metrics of the prediction / of the whole-foreground candidate
    src_lab_m, fg_lab_m = [], []    # label datasets: metrics of the fused per-label candidates of both sources
    fg_maps = []                    # region datasets: the whole-foreground candidates (host)
    with be.context():
        for name, pred, ref in cases:
            p, r = be.put(pred), be.put(ref)
            f = be.keep_largest(p, [fg_set])
            maps = [p, f]
            if per_step and not lm.has_regions:
                # Fused per-label candidates.  The step for label l only turns voxels of value l into background 0, and
                # 0 is no foreground label, so every other label's mask - its components, its counts, its Dice - is
                # the same whether step l ran or not.  One labelling of all labels as disjoint sets therefore gives
                # every label's candidate in any source the sequential loop can reach, and the source's own counts
                # give the baseline of each step.
                sets = [pp.label_set(l) for l in labels_or_regions]
                maps += [be.keep_largest(p, sets), be.keep_largest(f, sets)]
            ms = [ev.metrics_from_counts(c, labels_or_regions) for c in be.counts(r, maps, values, ignore)]
            base_m.append(ms[0])
            fg_m.append(ms[1])
            if len(ms) == 4:
                src_lab_m.append(ms[2])
                fg_lab_m.append(ms[3])
            if lm.has_regions:
                fg_maps.append(be.host(f))
            del p, r, f, maps

    baseline = _summary(base_m, names, labels_or_regions)
    fg_summary = _summary(fg_m, names, labels_or_regions)
    pp_fns, pp_fn_kwargs = [], []
    step = pp.remove_all_but_largest_component_from_segmentation
    if _fg_improves(baseline, fg_summary):
        say(f'Results were improved by removing all but the largest foreground region. Mean dice before: '
            f'{round(baseline["foreground_mean"]["Dice"], 5)} after: {round(fg_summary["foreground_mean"]["Dice"], 5)}')
        pp_fns.append(step)
        pp_fn_kwargs.append({'labels_or_regions': fg_labels})
        current, candidates, sources = fg_m, fg_lab_m, fg_maps
    else:
        say('Removing all but the largest foreground region did not improve results!')
        current, candidates, sources = base_m, src_lab_m, None
    current = [dict(m) for m in current]

    if per_step and not lm.has_regions:
        for l in labels_or_regions:
            before, after = _class_mean_dice(current, l), _class_mean_dice(candidates, l)
            if after > before:
                say(f'Results were improved by removing all but the largest component for {l}. '
                    f'Dice before: {round(before, 5)} after: {round(after, 5)}')
                for cur, cand in zip(current, candidates):
                    cur[l] = cand[l]
                pp_fns.append(step)
                pp_fn_kwargs.append({'labels_or_regions': l})
            else:
                say(f'Removing all but the largest component for {l} did not improve results!')
    elif per_step:
        # overlapping regions: the sequential loop, one labelling per region per case; the sources stay on the host
        if sources is None:
            sources = [_host_copy(p) for _, p, _ in cases]
        with be.context():
            for region in labels_or_regions:
                s = pp.label_set(region)
                cand_maps, cand_m = [], []
                for (name, _, ref), src in zip(cases, sources):
                    c = be.keep_largest(be.put(src), [s])
                    counts = be.counts(be.put(ref), [c], values, ignore)[0]
                    cand_m.append(ev.metrics_from_counts(counts, labels_or_regions))
                    cand_maps.append(be.host(c))
                before, after = _class_mean_dice(current, region), _class_mean_dice(cand_m, region)
                if after > before:
                    say(f'Results were improved by removing all but the largest component for {region}. '
                        f'Dice before: {round(before, 5)} after: {round(after, 5)}')
                    current, sources = cand_m, cand_maps
                    pp_fns.append(step)
                    pp_fn_kwargs.append({'labels_or_regions': region})
                else:
                    say(f'Removing all but the largest component for {region} did not improve results!')

    final = _summary(current, names, labels_or_regions)
    if output_folder is not None:
        _write_outputs(output_folder, baseline, final, pp_fns, pp_fn_kwargs)
        if save_postprocessed:
            for name, pred, _ in cases:
                out = be.apply(_host_copy(pred), pp_fns, pp_fn_kwargs)
                fname = name if name.endswith('.npy') else name + '.npy'
                np.save(os.path.join(output_folder, 'postprocessed', fname), np.asarray(out))
    # the reference hands back the kwargs after its JSON export turned numpy integers into Python ones (the pkl keeps
    # the numpy integers)
    return pp_fns, [ev.json_ready(k) for k in pp_fn_kwargs]
