"""Cross-configuration ensembling on the device (lifted: DESIGN.md section 6).

Mirrors the inference-time half of the reference's ``nnunetv2.ensembling.ensemble`` (ensembling/ensemble.py:16-44):

* ``average_probabilities`` - the float32 mean of several members' probabilities, in member order, bit for bit;
* ``ensemble_probabilities`` - ``merge_files`` without the image writer: that average and
  ``LabelManager.convert_logits_to_segmentation`` applied to it;
* ``nnUNetEnsemblePredictor`` - ``predict_single_npy_array`` and ``predict_from_files`` for an ensemble of
  configurations: every member preprocesses the raw case and runs its own sliding window, and one
  ``fnn_ensemble_resample_export`` call turns all members' network-grid logits into the averaged probabilities and the
  label map - without the ``.npz`` round trip and without a member's resampled logits ever being written (members whose
  plans resample at another order than 1 are resampled first and go through ``fnn_ensemble_export``: the same bytes).
  The file methods are the predictor's: the case loop of ``case_pipeline.run_pipeline`` with a reader and a writer
  thread, the case read and decoded once for all members.

``merge_files`` and ``ensemble_folders`` (ensemble.py:31-110) are the reference's folder commands on top of it: the members'
``.npz`` files are averaged on the device and the label file goes through the writer, one case at a time behind a reader
and a writer thread.
"""
from __future__ import annotations

import io
import os
import pickle
import shutil
from typing import List, Optional, Sequence, Union

import numpy as np
import torch

from . import capi
from .case_pipeline import as_plain_labels, compress_mode, export_case_files, labels_for_writer, run_pipeline
from .plans import label_rule
from .predictor import nnUNetPredictor

MAX_MEMBERS = 16


def _load_member(f) -> np.ndarray:
    if isinstance(f, (str, os.PathLike)):
        with np.load(f, allow_pickle=False) as z:          # object arrays raise ValueError here
            a = z['probabilities']
    else:
        a = np.asarray(f)
    if a.dtype not in (np.float32, np.float16):
        raise ValueError(f'probabilities must be float32 or float16, got {a.dtype}')
    return a


def _average_on_device(list_of_files_or_arrays, order, u16: bool, want_average: bool, device):
    assert len(list_of_files_or_arrays), 'At least one file must be given in list_of_files'
    if len(list_of_files_or_arrays) > MAX_MEMBERS:
        raise ValueError(f'at most {MAX_MEMBERS} members')
    device = torch.device(device) if device is not None else torch.device('cuda', torch.cuda.current_device())
    if device.type != 'cuda':
        raise RuntimeError('ensembling runs on the GPU; there is no CPU path')
    with torch.cuda.device(device):
        members, shape = [], None
        for f in list_of_files_or_arrays:
            a = _load_member(f)
            if shape is None:
                shape = a.shape
            elif a.shape != shape:
                raise ValueError(f'members have different shapes: {shape} and {a.shape}')
            members.append(torch.from_numpy(np.ascontiguousarray(a)).to(device=device, dtype=torch.float32))
        if len(shape) < 2:
            raise ValueError('probabilities must have shape (c, x, y(, z))')
        heads, n_vox = int(shape[0]), int(np.prod(shape[1:]))
        if order is not None and len(order) != heads:
            raise ValueError(f'{heads} channels, but {len(order)} entries in regions_class_order')
        avg = torch.empty(shape, dtype=torch.float32, device=device) if want_average else None
        labels = torch.empty(shape[1:], dtype=torch.int16 if u16 else torch.uint8, device=device)
        capi.average_probabilities([m.data_ptr() for m in members], heads, order, n_vox,
                                   None if avg is None else avg.data_ptr(), labels.data_ptr(), u16,
                                   torch.cuda.current_stream(device).cuda_stream)
    return avg, labels


@torch.inference_mode()
def average_probabilities(list_of_files_or_arrays: List[Union[str, np.ndarray]], device=None) -> np.ndarray:
    """ensemble.py:16-28: ``.npz`` files (their ``probabilities``, loaded without pickle) or arrays -> float32 mean,
    bit-identical to the reference's numpy loop (p_0 in float32, += p_i in order, /= n)."""
    avg, _ = _average_on_device(list_of_files_or_arrays, None, False, True, device)
    return avg.cpu().numpy()


@torch.inference_mode()
def ensemble_probabilities(list_of_files_or_arrays: List[Union[str, np.ndarray]], label_manager,
                           return_probabilities: bool = False, device=None):
    """``merge_files`` (ensemble.py:31-44) without the image writer: -> label map (uint8, or uint16 with 255 or more
    foreground labels), and ``(labels, average)`` with ``return_probabilities``.  For region-based training the
    reference applies the sigmoid to the averaged probabilities again before ``> 0.5``; so does this."""
    order, u16 = label_rule(label_manager)
    avg, labels = _average_on_device(list_of_files_or_arrays, order, u16, return_probabilities, device)
    labels = labels.cpu().numpy().view(np.uint16) if u16 else labels.cpu().numpy()
    return (labels, avg.cpu().numpy()) if return_probabilities else labels


def _label_signature(lm):
    return (bool(lm.has_regions), None if lm.regions_class_order is None else [int(c) for c in lm.regions_class_order],
            list(lm.all_labels), lm.all_regions, int(lm.num_segmentation_heads), lm.ignore_label)


class nnUNetEnsemblePredictor(object):
    """An ensemble of initialised ``nnUNetPredictor`` members (e.g. ``2d`` + ``3d_fullres``, or ``3d_fullres`` +
    ``3d_lowres``, as ``nnUNetv2_find_best_configuration`` picks them), predicted on the device: arrays
    (``predict_single_npy_array``) or files (``predict_from_files``, ``predict_from_files_sequential``).

    fused_export  the step from the members' logits to the ensemble's labels is one ``fnn_ensemble_resample_export`` call
                  on the members' network-grid logits whenever every member's plan allows it (``plan_ensemble_export``:
                  order-1 default plans, torch-resampling plans, equal grids); False, or a member that resamples at another
                  order: every member's logits are resampled to the cropped grid first and ``fnn_ensemble_export`` reads
                  those - the same bytes.  ``export_stats`` counts the cases by the route they took.
    compress_on_device  as ``nnUNetPredictor``'s (False, True or ``'dynamic'``): the ensemble's label file is compressed on
                  the GPU.

    Memory: the fused step keeps only the members' network-grid logits resident (N x heads x network-grid voxels x 2 B; a
    ``3d_lowres`` member at twice the spacing is an eighth of the cropped grid).  The two-step route keeps the members'
    resampled fp16 logits resident at the same time - N x heads x cropped voxels x 2 B (two members of a 61-class 512^3
    case: 32.7 GB) - on top of one member's network-grid logits while it runs."""

    def __init__(self, predictors: Sequence[nnUNetPredictor], fused_export: bool = True, compress_on_device=False):
        predictors = list(predictors)
        if not 1 <= len(predictors) <= MAX_MEMBERS:
            raise ValueError(f'an ensemble has 1..{MAX_MEMBERS} members, got {len(predictors)}')
        for p in predictors:
            if not isinstance(p, nnUNetPredictor) or p.label_manager is None or p.plans_manager is None:
                raise ValueError('every member must be an initialised nnUNetPredictor')
        first = predictors[0]
        for p in predictors[1:]:
            if p.device != first.device:
                raise ValueError(f'members on different devices: {first.device} and {p.device}')
            if _label_signature(p.label_manager) != _label_signature(first.label_manager):
                raise ValueError('members have different labels / regions: they cannot be averaged')
            if [int(i) for i in p.plans_manager.transpose_forward] != [int(i) for i in first.plans_manager.transpose_forward]:
                raise ValueError('members have different transpose_forward: their crops live on different grids')
        self.predictors = predictors
        self.device = first.device
        self.label_manager = first.label_manager
        self.plans_manager = first.plans_manager
        self.dataset_json = first.dataset_json
        self.verbose = first.verbose
        self.fused_export = bool(fused_export)
        self.compress_on_device = compress_mode(compress_on_device)
        self.export_stats = {'fused': 0, 'two-step': 0}
        self._postprocessing = None
        self._rw = None

    def set_postprocessing(self, postprocessing):
        """As ``nnUNetPredictor.set_postprocessing``: applied to the ensemble's device label map on the raw grid
        before it is copied to the host; probabilities are never changed."""
        nnUNetPredictor.set_postprocessing(self, postprocessing)

    @torch.inference_mode()
    def predict_single_npy_array(self, input_image: np.ndarray, image_properties: dict,
                                 segmentation_previous_stage: Optional[Sequence[Optional[np.ndarray]]] = None,
                                 output_file_truncated: str = None, save_or_return_probabilities: bool = False):
        """Raw image ``[C, s0, s1, s2]`` + ``{'spacing': ...}`` -> ensembled label map on the raw grid (numpy, uint8 /
        uint16), or ``(labels, float32 average probabilities [heads, s0, s1, s2])`` with
        ``save_or_return_probabilities``: what ``merge_files`` makes of the members' exported probabilities.
        ``segmentation_previous_stage``: None, or one entry per member (None for members that are no cascade stage).
        Files are written by ``predict_from_files``."""
        if output_file_truncated is not None:
            raise NotImplementedError('predict_single_npy_array returns arrays; predict_from_files writes image files')
        seg, avg, _ = self._predict_case(input_image, image_properties, segmentation_previous_stage,
                                         save_or_return_probabilities)
        return (seg, avg) if save_or_return_probabilities else seg

    def _predict_case(self, input_image, image_properties: dict, segmentation_previous_stage=None,
                      save_or_return_probabilities: bool = False, for_file: bool = False):
        """-> (labels on the raw grid as ``_labels_out`` makes them, float32 average or None, the case's properties after
        preprocessing).  ``input_image`` is a numpy array or a tensor (a resident one stays where it is): every member
        preprocesses the same one."""
        from .preprocess import case_label_export_plan, plan_ensemble_export
        n = len(self.predictors)
        prev = [None] * n if segmentation_previous_stage is None else list(segmentation_previous_stage)
        if len(prev) != n:
            raise ValueError(f'segmentation_previous_stage: {len(prev)} entries for {n} members')
        cases, props0 = [], None
        for p, sp in zip(self.predictors, prev):
            pp, data, props = p._preprocess_case(input_image, image_properties, sp)
            if props0 is None:
                props0 = props
            elif [list(map(int, b)) for b in props['bbox_used_for_cropping']] != \
                    [list(map(int, b)) for b in props0['bbox_used_for_cropping']] or \
                    tuple(props['shape_after_cropping_and_before_resampling']) != \
                    tuple(props0['shape_after_cropping_and_before_resampling']) or \
                    tuple(props['shape_before_cropping']) != tuple(props0['shape_before_cropping']):
                raise RuntimeError('members cropped the case differently: their probabilities cannot be averaged')
            cases.append((p, pp, data, props,
                          case_label_export_plan(data.shape[1:], p.plans_manager, p.configuration_manager, props)))
        fused = self.fused_export and plan_ensemble_export([c[4] for c in cases]) == 'fused'
        resident = []
        while cases:
            p, pp, data, props, plan = cases.pop(0)
            if self.verbose:
                print('predicting')
            logits = p._predict_case_logits(data)
            del data
            if not fused:
                logits = pp.resample_logits_to_cropped_shape(logits, p.plans_manager, p.configuration_manager, props)
            resident.append((logits, plan))
        labels, avg = self._export_members(resident, fused, props0, save_or_return_probabilities)
        del resident
        out = nnUNetPredictor._labels_out(self, as_plain_labels(labels), props0, for_file=for_file)
        return out, None if avg is None else avg.cpu().numpy(), props0

    def _export_members(self, resident, fused: bool, props0: dict, want_average: bool):
        """The step from the members' logits to the ensemble's labels: ``resident`` holds one (logits, label-export plan)
        per member - network-grid logits when ``fused``, else logits of the cropped grid.  -> (device labels on the raw
        grid, device float32 average or None)."""
        order, u16 = label_rule(self.label_manager)
        before = [int(i) for i in props0['shape_before_cropping']]
        cropped = [int(i) for i in props0['shape_after_cropping_and_before_resampling']]
        tb = [int(i) for i in self.plans_manager.transpose_backward]
        grid = [before[j] for j in tb]
        with torch.cuda.device(self.device):
            lgs = [lg.contiguous() for lg, _ in resident]
            heads = lgs[0].shape[0]
            avg = torch.empty((heads, *grid), dtype=torch.float32, device=self.device) if want_average else None
            labels = torch.empty(grid, dtype=torch.int16 if u16 else torch.uint8, device=self.device)
            stream = torch.cuda.current_stream(self.device).cuda_stream
            avg_ptr = None if avg is None else avg.data_ptr()
            if fused:
                members = []
                for lg, (_, plan) in zip(lgs, resident):
                    if plan['path'] == 'same-grid' and [int(i) for i in lg.shape[1:]] != cropped:
                        raise RuntimeError(f'logits of shape {tuple(lg.shape[1:])} are not resampled, the crop is {cropped}')
                    members.append((lg.data_ptr(), lg.dtype == torch.half, lg.shape[1:],
                                    capi.FNN_RESAMPLE_TORCH if plan['path'] == 'fused-torch' else capi.FNN_RESAMPLE_DEFAULT,
                                    plan['separate_axis']))
                capi.ensemble_resample_export(members, heads, order, props0['bbox_used_for_cropping'], before, tb, avg_ptr,
                                              labels.data_ptr(), u16, stream)
            else:
                capi.ensemble_export([lg.data_ptr() for lg in lgs], [lg.dtype == torch.half for lg in lgs], heads, order,
                                     props0['bbox_used_for_cropping'], before, tb, avg_ptr, labels.data_ptr(), u16, stream)
        self.export_stats['fused' if fused else 'two-step'] += 1
        return labels, avg

    # ----------------------------------------------------------------- files
    # what a predictor and an ensemble do alike around the cases of a files run is nnUNetPredictor's
    _label_files = nnUNetPredictor._label_files
    _labels_out = nnUNetPredictor._labels_out
    _export_case = nnUNetPredictor._export_case
    _result = staticmethod(nnUNetPredictor._result)
    predict_from_files = nnUNetPredictor.predict_from_files
    predict_from_files_sequential = nnUNetPredictor.predict_from_files_sequential

    def _reader_writer(self):
        """One instance of the members' common reader-writer class (``nnUNetPredictor._reader_writer``); members that read
        or write differently are a ValueError."""
        if self._rw is None:
            from .imageio import prediction_reader_writer_class
            classes = [prediction_reader_writer_class(p.plans_manager, p.dataset_json) for p in self.predictors]
            if any(c is not classes[0] for c in classes):
                raise ValueError(f'members read and write images differently: {sorted({c.__name__ for c in classes})}')
            self._rw = classes[0](self.device)
        return self._rw

    def _prepare_files_run(self, call_kwargs: dict, sequential: bool):
        """``nnUNetPredictor._prepare_files_run`` behind what only an ensemble can get wrong: members of different file
        types, and previous-stage folders that are not one per member."""
        endings = sorted({str(p.dataset_json['file_ending']) for p in self.predictors})
        if len(endings) > 1:
            raise ValueError(f'members have different file endings: {endings}')
        folders = call_kwargs.get('folder_with_segs_from_prev_stage')
        if folders is not None and (isinstance(folders, (str, os.PathLike)) or len(folders) != len(self.predictors)):
            raise ValueError(f'folder_with_segs_from_prev_stage: None, or one entry per member ({len(self.predictors)}; None for '
                             f'members that are no cascade stage)')
        self._reader_writer()
        return nnUNetPredictor._prepare_files_run(self, call_kwargs, sequential)

    def _assert_prev_stage_folder(self, folders):
        for p, folder in zip(self.predictors, folders if folders is not None else [None] * len(self.predictors)):
            p._assert_prev_stage_folder(folder)

    def _manage_input_and_output_lists(self, list_of_lists_or_source_folder, output_folder_or_list_of_truncated_output_files,
                                       folder_with_segs_from_prev_stage=None, overwrite: bool = True, part_id: int = 0,
                                       num_parts: int = 1, save_probabilities: bool = False):
        """``nnUNetPredictor._manage_input_and_output_lists`` with the previous stage's files per member: the third list
        holds, per case, None or one file name (or None) per member."""
        cases, truncated, _ = nnUNetPredictor._manage_input_and_output_lists(
            self, list_of_lists_or_source_folder, output_folder_or_list_of_truncated_output_files, None, overwrite,
            part_id, num_parts, save_probabilities)
        if folder_with_segs_from_prev_stage is None or all(f is None for f in folder_with_segs_from_prev_stage):
            return cases, truncated, [None] * len(cases)
        ending = self.dataset_json['file_ending']
        caseids = [os.path.basename(c[0])[:-(len(ending) + 5)] for c in cases]
        return cases, truncated, [[None if f is None else os.path.join(f, i + ending) for f in folder_with_segs_from_prev_stage]
                                  for i in caseids]

    @torch.inference_mode()
    def _predict_cases(self, cases, truncated, prev, save_probabilities, read_thread: bool, write_thread: bool):
        """The case loop of ``nnUNetPredictor._predict_cases`` with one previous-stage file per cascade member: the case is
        read and decoded once, every member preprocesses that device tensor."""
        rw = self._reader_writer()                              # (made by the calling thread)
        if truncated is None:
            truncated = [None] * len(cases)
        n_slots = len(self.predictors) + 1

        def stage(i):
            slot = n_slots * (i % 2)
            staged = rw.stage(cases[i], slot=slot)
            staged_prev = [None if f is None else rw.stage([f], slot=slot + 1 + m) for m, f in enumerate(prev[i] or [])]
            return lambda: (staged.fill(), [None if s is None else s.fill() for s in staged_prev])

        def run(i, filled):
            staged, staged_prev = filled
            data, props = rw.decode(staged)
            seg_prev = [None if s is None else rw.decode(s)[0] for s in staged_prev] or None
            if staged.fnames and self.verbose:
                print(f'predicting {os.path.basename(staged.fnames[0])}')
            seg, avg, props = self._predict_case(data, props, seg_prev, save_probabilities, for_file=truncated[i] is not None)
            if truncated[i] is None:
                return self._result(seg, avg, save_probabilities), None
            return None, (lambda: self._export_case(seg, avg, props, truncated[i]))

        return run_pipeline(len(cases), stage, run, read_thread, write_thread)


# ---- folders -----------------------------------------------------------------------------------------------------------
class _PropertiesUnpickler(pickle.Unpickler):
    """Reads the properties ``.pkl`` next to a member's ``.npz`` without running what it names: numpy arrays and scalars of
    plain numeric dtypes and builtin containers are rebuilt, every other global is refused."""
    _MULTIARRAY = ('numpy.core.multiarray', 'numpy._core.multiarray')
    _BUILTINS = {'set': set, 'frozenset': frozenset, 'slice': slice, 'complex': complex, 'bytearray': bytearray, 'range': range}

    def find_class(self, module, name):
        if (module, name) == ('numpy', 'ndarray'):
            return np.ndarray
        if (module, name) == ('numpy', 'dtype'):
            return _plain_dtype
        if module in self._MULTIARRAY and name == '_reconstruct':
            return _reconstruct_array
        if module in self._MULTIARRAY and name == 'scalar':
            return _plain_scalar
        if module == 'builtins' and name in self._BUILTINS:
            return self._BUILTINS[name]
        if (module, name) == ('collections', 'OrderedDict'):
            import collections
            return collections.OrderedDict
        raise pickle.UnpicklingError(f'the properties pickle names a global that is not allowed: {module}.{name}')


def _plain_dtype(*args, **kwargs):
    dt = np.dtype(*args, **kwargs)
    if dt.hasobject or dt.kind not in 'biufc':
        raise pickle.UnpicklingError(f'numpy dtype {dt} is not allowed in a properties pickle')
    return dt


def _reconstruct_array(cls, shape, typecode):
    if cls is not np.ndarray:
        raise pickle.UnpicklingError('only plain numpy arrays are allowed in a properties pickle')
    return np.ndarray.__new__(np.ndarray, shape, typecode)


def _plain_scalar(dtype, data=None):
    dtype = np.dtype(dtype)
    if dtype.kind not in 'biuf' or data is None:
        raise pickle.UnpicklingError(f'numpy scalar of dtype {dtype} is not allowed in a properties pickle')
    return np.frombuffer(data, dtype=dtype, count=1)[0]


def load_properties_pkl(path_or_bytes) -> dict:
    """The properties a prediction was exported with (``<case>.pkl`` next to ``<case>.npz``), loaded without pickle's
    freedom to import and call."""
    if isinstance(path_or_bytes, (bytes, bytearray)):
        data = bytes(path_or_bytes)
    else:
        with open(path_or_bytes, 'rb') as f:
            data = f.read()
    return _PropertiesUnpickler(io.BytesIO(data)).load()


def _merge_on_device(members, properties, image_reader_writer, label_manager, save_probabilities: bool):
    """The GPU part of ``merge_files`` -> (what the writer takes as the label map, the average on the host or None)."""
    order, u16 = label_rule(label_manager)
    avg, labels = _average_on_device(members, order, u16, save_probabilities, None)
    if labels.ndim != 3:
        raise ValueError(f'probabilities of shape {tuple(avg.shape) if avg is not None else labels.shape}: the label file needs (c, z, y, x)')
    return labels_for_writer(image_reader_writer, labels, properties), None if avg is None else avg.cpu().numpy()


@torch.inference_mode()
def merge_files(list_of_files: Sequence[str], output_filename_truncated: str, output_file_ending: str, image_reader_writer,
                label_manager, save_probabilities: bool = False):
    """``merge_files`` (ensemble.py:31-45): the properties of the first member's ``.pkl``, the members' ``.npz`` averaged and
    turned into labels on the device, the label file through the writer.  With ``save_probabilities`` the average goes to
    ``.npz`` and the *properties* to ``.pkl`` (the reference pickles the probability array there, which no reader of that
    pair expects)."""
    list_of_files = [str(f) for f in list_of_files]
    properties = load_properties_pkl(list_of_files[0][:-4] + '.pkl')
    seg, avg = _merge_on_device(list_of_files, properties, image_reader_writer, label_manager, save_probabilities)
    export_case_files(output_filename_truncated, avg, properties, lambda: image_reader_writer.write_seg(
        seg, output_filename_truncated + output_file_ending, properties))


@torch.inference_mode()
def ensemble_folders(list_of_input_folders: List[str], output_folder: str, save_merged_probabilities: bool = False,
                     num_processes: int = 8, dataset_json_file_or_dict=None, plans_json_file_or_dict=None):
    """``ensemble_folders`` (ensemble.py:48-110).  If plans and dataset json are not specified, those of the first folder are
    taken.  The members are the folders' ``.npz`` files and every folder must hold the same set.  A reader thread loads the
    next case's members and a writer thread writes the previous case's files while the calling thread averages this one on
    the device; ``num_processes`` is accepted and ignored."""
    from .label_folders import folder_plans_and_dataset, subfiles
    plans_manager, dataset_json, rw = folder_plans_and_dataset(list_of_input_folders[0], plans_json_file_or_dict,
                                                               dataset_json_file_or_dict)
    files_per_folder = [set(subfiles(i, suffix='.npz', join=False)) for i in list_of_input_folders]
    s = set(files_per_folder[0])
    for f in files_per_folder[1:]:
        s.update(f)
    for f in files_per_folder:
        assert len(s.difference(f)) == 0, 'Not all folders contain the same files for ensembling. Please only ' \
                                          'provide folders that contain the predictions'
    names = sorted(s)
    lists_of_lists_of_files = [[os.path.join(fl, fi) for fl in list_of_input_folders] for fi in names]
    output_files_truncated = [os.path.join(output_folder, fi[:-4]) for fi in names]
    label_manager = plans_manager.get_label_manager(dataset_json)
    os.makedirs(output_folder, exist_ok=True)
    shutil.copy(os.path.join(list_of_input_folders[0], 'dataset.json'), output_folder)
    ending = dataset_json['file_ending']

    def stage(i):
        files = lists_of_lists_of_files[i]
        return lambda: ([_load_member(f) for f in files], load_properties_pkl(files[0][:-4] + '.pkl'))

    def run(i, data):
        members, properties = data
        seg, avg = _merge_on_device(members, properties, rw, label_manager, save_merged_probabilities)
        return None, (lambda: export_case_files(output_files_truncated[i], avg, properties, lambda: rw.write_seg(
            seg, output_files_truncated[i] + ending, properties)))

    run_pipeline(len(names), stage, run, write_thread=True)
