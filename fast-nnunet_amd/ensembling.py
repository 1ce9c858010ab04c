"""Cross-configuration ensembling on the device (lifted: DESIGN.md section 6).

Mirrors the inference-time half of the reference's ``nnunetv2.ensembling.ensemble`` (ensembling/ensemble.py:16-44):

* ``average_probabilities`` - the float32 mean of several members' probabilities, in member order, bit for bit;
* ``ensemble_probabilities`` - ``merge_files`` without the image writer: that average and
  ``LabelManager.convert_logits_to_segmentation`` applied to it;
* ``nnUNetEnsemblePredictor`` - ``predict_single_npy_array`` for an ensemble of configurations: every member
  preprocesses the raw case and runs its own sliding window, and one ``fnn_ensemble_export`` call turns all members'
  resampled logits into the averaged probabilities and the label map, without the ``.npz`` round trip.

``merge_files`` and ``ensemble_folders`` (ensemble.py:31-110) are the reference's folder commands on top of it: the members'
``.npz`` files are averaged on the device and the label file goes through the writer, one case at a time behind a reader
and a writer thread.  File output on ``nnUNetEnsemblePredictor`` stays out.
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
from .case_pipeline import as_plain_labels, export_case_files, labels_for_writer, run_pipeline
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
    ``3d_lowres``, as ``nnUNetv2_find_best_configuration`` picks them), predicted on the device.

    Memory: the members' resampled fp16 logits are resident at the same time - N x heads x cropped voxels x 2 B (two
    members of a 61-class 512^3 case: 32.7 GB) - on top of one member's network-grid logits while it runs; a member's
    network-grid logits are freed once they are resampled."""

    def __init__(self, predictors: Sequence[nnUNetPredictor]):
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
        self.verbose = first.verbose
        self._postprocessing = None

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
        ``segmentation_previous_stage``: None, or one entry per member (None for members that are no cascade stage)."""
        if output_file_truncated is not None:
            raise NotImplementedError('image file export is the caller\'s side (SURVEY.md 8: image I/O out of scope)')
        n = len(self.predictors)
        prev = [None] * n if segmentation_previous_stage is None else list(segmentation_previous_stage)
        if len(prev) != n:
            raise ValueError(f'segmentation_previous_stage: {len(prev)} entries for {n} members')
        resident, props0 = [], None
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
            if self.verbose:
                print('predicting')
            logits = p._predict_case_logits(data)
            del data
            resident.append(pp.resample_logits_to_cropped_shape(logits, p.plans_manager, p.configuration_manager, props))
            del logits
        order, u16 = label_rule(self.label_manager)
        before = [int(i) for i in props0['shape_before_cropping']]
        tb = [int(i) for i in self.plans_manager.transpose_backward]
        grid = [before[j] for j in tb]
        with torch.cuda.device(self.device):
            resident = [lg.contiguous() for lg in resident]
            avg = torch.empty((resident[0].shape[0], *grid), dtype=torch.float32, device=self.device) \
                if save_or_return_probabilities else None
            labels = torch.empty(grid, dtype=torch.int16 if u16 else torch.uint8, device=self.device)
            capi.ensemble_export([lg.data_ptr() for lg in resident], [lg.dtype == torch.half for lg in resident],
                                 resident[0].shape[0], order, props0['bbox_used_for_cropping'], before, tb,
                                 None if avg is None else avg.data_ptr(), labels.data_ptr(), u16,
                                 torch.cuda.current_stream(self.device).cuda_stream)
            del resident
        out = nnUNetPredictor._labels_out(self, as_plain_labels(labels), props0, for_file=False)
        if save_or_return_probabilities:
            return out, avg.cpu().numpy()
        return out


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
