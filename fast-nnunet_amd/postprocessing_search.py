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

``determine_postprocessing_on_folder`` is the reference's function itself, on folders of label files: the same search fed
by ``FolderBackend``, which reads a case's files as labels on the device when the search asks for them (a reader thread
inflates the next case's meanwhile) and keeps the candidates the search holds between steps deflated on the host.
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
from .case_pipeline import HostWorker, as_plain_labels
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


class LabelFile:
    """A label file that stands in for its map in ``determine_postprocessing``: the header's shape now, the labels when
    ``FolderBackend.put`` reads them."""

    def __init__(self, fname: str):
        from .imageio import read_header
        self.fname = str(fname)
        self.shape = tuple(read_header(self.fname).shape)


class PackedLabels:
    """A label map between two steps of the search, deflated (level 1) on the host."""

    def __init__(self, arr: np.ndarray):
        import zlib
        arr = np.ascontiguousarray(arr)
        self.shape, self.dtype = arr.shape, arr.dtype
        self.blob = zlib.compress(memoryview(arr).cast('B'), 1)

    def array(self) -> np.ndarray:
        import zlib
        return np.frombuffer(bytearray(zlib.decompress(self.blob)), dtype=self.dtype).reshape(self.shape)


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
        for m in (p, r):
            if not isinstance(m, LabelFile):                     # (a file is checked by the kernel that decodes it)
                ev.check_label_map(m)
        out.append((n, p, r))
    return out


def _device_map(seg, dev: torch.device) -> torch.Tensor:
    """A device copy the labelling kernel can take (uint8 stays uint8, any other integer type becomes int32)."""
    if isinstance(seg, torch.Tensor):
        t = seg.to(dev)
        return t if t.dtype == torch.uint8 else t.to(torch.int32)
    arr = np.asarray(seg)
    return torch.from_numpy(np.ascontiguousarray(arr if arr.dtype == np.uint8 else arr.astype(np.int32))).to(dev)


def _host_copy(seg):
    if isinstance(seg, (LabelFile, PackedLabels)):               # (immutable: the search never writes its sources)
        return seg
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


def _write_outputs(output_folder: str, baseline: dict, final: dict, pp_fns, pp_fn_kwargs, write_baseline: bool = True,
                   write_final: bool = True):
    os.makedirs(output_folder, exist_ok=True)
    if write_baseline:
        ev.save_summary_json(baseline, os.path.join(output_folder, 'summary.json'))
    if write_final:
        os.makedirs(os.path.join(output_folder, 'postprocessed'), exist_ok=True)
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
        return pp._postprocess(seg, [pp.GpuPass('largest', sets, 0)])

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
    cases, pp_fns, pp_fn_kwargs, baseline, final, be = _search(predictions, references, dataset_json_or_label_manager, verbose,
                                                               backend)
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


def _search(predictions, references, dataset_json_or_label_manager, verbose: bool = False, backend=None,
            baseline: Optional[dict] = None):
    """The search itself -> (cases, pp_fns, pp_fn_kwargs with numpy integers, baseline summary, final summary, backend).
    ``baseline``: a summary of the predictions made earlier (the reference reuses an existing summary.json); its per-case
    metrics then stand for the ones counted here."""
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
    begin_pass = getattr(be, 'begin_pass', lambda sources, refs: None)   # (a backend that reads ahead learns the order)
    names = [n for n, _, _ in cases]
    values = ev.count_classes(labels_or_regions)
    fg_set = pp.label_set(list(fg_labels))
    per_step = len(labels_or_regions) > 1
    say = print if verbose else (lambda *a, **k: None)

    base_m, fg_m = [], []           # per case: metrics of the prediction / of the whole-foreground candidate
    src_lab_m, fg_lab_m = [], []    # label datasets: metrics of the fused per-label candidates of both sources
    fg_maps = []                    # region datasets: the whole-foreground candidates (host)
    with be.context():
        begin_pass([p for _, p, _ in cases], [r for _, _, r in cases])
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

    if baseline is None:
        baseline = _summary(base_m, names, labels_or_regions)
    else:
        if len(baseline['metric_per_case']) != len(cases):
            raise ValueError(f"the summary given as baseline has {len(baseline['metric_per_case'])} cases, the folder {len(cases)}")
        base_m = [c['metrics'] for c in baseline['metric_per_case']]
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
                begin_pass(sources, [r for _, _, r in cases])
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
    return cases, pp_fns, pp_fn_kwargs, baseline, final, be


class FolderBackend(DeviceBackend):
    """``DeviceBackend`` for sources that are label files (``LabelFile``) or deflated maps (``PackedLabels``): ``put`` reads a
    file as labels on the device (``decode_label_maps``); ``begin_pass`` tells it the order in which a pass over the cases
    will ask, so that one ``HostWorker`` inflates the files of the next case into the other slot of pinned buffers while
    this one runs; ``host`` deflates what the search keeps between steps.  One case is on the device at a time and the
    folder is never in host memory as a whole.  Used as a context manager: the reader thread lives inside the ``with``."""

    def __init__(self, rw):
        DeviceBackend.__init__(self)
        self.rw = rw
        self.reader = None
        self.plan, self.at, self.job, self.ready = [], 0, None, {}

    def __enter__(self):
        self.reader = HostWorker('fnn-reader')
        return self

    def __exit__(self, *exc):
        if self.reader is not None:
            self.reader.close()
            self.reader = None

    def _submit(self, k: int):
        files = self.plan[k]
        if not files:
            return None
        return self.reader.submit(self.rw.stage_label_files(files, slot=k % 2).fill)

    def begin_pass(self, sources, refs):
        if self.job is not None:
            self.job.done.wait()                                 # (nothing of an abandoned pass stays in flight)
        self.plan = [[m.fname for m in pair if isinstance(m, LabelFile)] for pair in zip(sources, refs)]
        self.at, self.ready = 0, {}
        self.job = self._submit(0) if self.plan else None

    def _read(self, fname: str):
        if fname not in self.ready and self.at < len(self.plan) and fname in self.plan[self.at]:
            staged = self.job.result()
            self.at += 1
            self.job = self._submit(self.at) if self.at < len(self.plan) else None
            self.ready = {f: m for f, (m, _) in zip(staged.fnames, self.rw.decode_label_maps(staged))}
        if fname in self.ready:
            return self.ready.pop(fname)
        # asked out of order: read here and now, through a slot of pinned buffers that the reader thread never fills
        return self.rw.decode_label_maps(self.rw.stage_label_files([fname], slot=2).fill())[0][0]

    def put(self, seg):
        if isinstance(seg, LabelFile):
            return as_plain_labels(self._read(seg.fname))
        if isinstance(seg, PackedLabels):
            seg = seg.array()
        return DeviceBackend.put(self, seg)

    def host(self, seg):
        return PackedLabels(seg.cpu().numpy())


def determine_postprocessing_on_folder(folder_predictions: str, folder_ref: str, plans_file_or_dict=None,
                                       dataset_json_file_or_dict=None, num_processes: int = 8,
                                       keep_postprocessed_files: bool = True, verbose: bool = True,
                                       inflate_on_device=False):
    """The reference's ``determine_postprocessing`` (remove_connected_components.py:52-244) on folders of label files.

    Leaves what the reference leaves: ``summary.json`` in ``folder_predictions`` (an existing one is reused, as the
    reference reuses it), ``postprocessing.pkl``, ``postprocessing.json``, and - unless ``keep_postprocessed_files`` is
    False - ``postprocessed/<files>`` with ``postprocessed/summary.json``; no ``temp`` folder is made.  Plans or
    dataset.json given as None are looked for in ``folder_predictions``.  ``num_processes`` is accepted and ignored.
    ``inflate_on_device``: predictions written with ``compress_on_device=True``, which the search reads several times, are
    inflated on the GPU (``NiftiIO(inflate_on_device=True)``; ``'dynamic'``: those written with
    ``compress_on_device='dynamic'`` too).  Returns ``(pp_fns, pp_fn_kwargs)``."""
    from .label_folders import folder_plans_and_dataset, subfiles
    missing = 'Expected plans file missing: {}. The plans files should have been created while running nnUNetv2_predict. Sadge.'
    plans_manager, dataset_json, rw = folder_plans_and_dataset(folder_predictions, plans_file_or_dict,
                                                               dataset_json_file_or_dict, missing, missing,
                                                               inflate_on_device=inflate_on_device)
    ending = dataset_json['file_ending']
    predicted_files = subfiles(folder_predictions, suffix=ending, join=False)
    ref_files = subfiles(folder_ref, suffix=ending, join=False)
    if not all(i in predicted_files for i in ref_files):
        print('WARNING: Not all files in folder_ref were found in folder_predictions. Determining postprocessing '
              'should always be done on the entire dataset!')
    if not predicted_files:
        raise ValueError(f'no {ending} file in {folder_predictions}')
    missing = [i for i in predicted_files if not os.path.isfile(os.path.join(folder_ref, i))]
    if missing:
        raise ValueError(f'predictions without a reference: {missing[:5]}')
    summary_file = os.path.join(folder_predictions, 'summary.json')
    known = ev.load_summary_json(summary_file) if os.path.isfile(summary_file) else None
    preds = {i: LabelFile(os.path.join(folder_predictions, i)) for i in predicted_files}
    refs = {i: LabelFile(os.path.join(folder_ref, i)) for i in predicted_files}
    with FolderBackend(rw) as be:
        _, pp_fns, pp_fn_kwargs, baseline, final, _ = _search(preds, refs, plans_manager.get_label_manager(dataset_json),
                                                              verbose, be, baseline=known)
    output_folder = os.path.join(folder_predictions, 'postprocessed')
    if known is None:
        for case, name in zip(baseline['metric_per_case'], predicted_files):
            case['reference_file'] = os.path.join(folder_ref, name)
            case['prediction_file'] = os.path.join(folder_predictions, name)
    for case, name in zip(final['metric_per_case'], predicted_files):
        case['reference_file'] = os.path.join(folder_ref, name)
        case['prediction_file'] = os.path.join(output_folder, name)
    _write_outputs(folder_predictions, baseline, final, pp_fns, pp_fn_kwargs, write_baseline=known is None,
                   write_final=keep_postprocessed_files)
    if keep_postprocessed_files:
        pp.apply_postprocessing_to_files([os.path.join(folder_predictions, i) for i in predicted_files],
                                         [os.path.join(output_folder, i) for i in predicted_files], rw, pp_fns, pp_fn_kwargs)
    return pp_fns, [ev.json_ready(k) for k in pp_fn_kwargs]
