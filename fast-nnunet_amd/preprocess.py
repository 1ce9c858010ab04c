"""Whole-volume steps on either side of the sliding window, on the device.

Mirrors, with the reference's argument names and property keys,

* ``DefaultPreprocessor.run_case_npy`` (preprocessing/preprocessors/default_preprocessor.py:45-118) up to - and
  excluding - the resampling call: float32 copy, ``transpose_forward``, ``crop_to_nonzero``, per-channel intensity
  normalisation, then ``resample_data_or_seg_to_shape`` to the configuration's spacing
  (preprocessing/resampling/default_resampling.py:88-196: per-channel order-3 ``resize``, or per-slice resize + an
  order-0 pass along the anisotropic axis);
* ``convert_predicted_logits_to_segmentation_with_correct_shape`` (inference/export_prediction.py:16-53): logits
  resampled back to ``shape_after_cropping_and_before_resampling`` (order 1 by default), label rule, dtype rule,
  revert cropping, ``transpose_backward``.

Every numerical step is a HIP kernel behind ``include/fnn.h`` (``fnn_nonzero_bbox``, ``fnn_preprocess``,
``fnn_resample``, ``fnn_resample_torch``, ``fnn_resample_torch_seg``, ``fnn_resample_labels``, ``fnn_argmax_labels``,
``fnn_revert_labels``); torch only owns the device buffers.  No CPU path.
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import capi
from .case_pipeline import as_plain_labels
from .plans import label_rule

_SCHEMES = {'NoNormalization': capi.FNN_NORM_NONE, 'ZScoreNormalization': capi.FNN_NORM_ZSCORE,
            'CTNormalization': capi.FNN_NORM_CT, 'RescaleTo01Normalization': capi.FNN_NORM_RESCALE01,
            'RGBTo01Normalization': capi.FNN_NORM_RGB01}


ANISO_THRESHOLD = 3           # nnunetv2/configuration.py


def determine_do_sep_z_and_axis(force_separate_z, current_spacing, new_spacing,
                                separate_z_anisotropy_threshold: float = ANISO_THRESHOLD):
    """preprocessing/resampling/default_resampling.py:14-71."""
    def aniso(sp):
        return (np.max(sp) / np.min(sp)) > separate_z_anisotropy_threshold

    def lowres_axis(sp):
        return np.where(max(sp) / np.array(sp) == 1)[0]

    if force_separate_z is not None:
        do_separate_z = force_separate_z
        axis = lowres_axis(current_spacing) if force_separate_z else None
    elif aniso(current_spacing):
        do_separate_z, axis = True, lowres_axis(current_spacing)
    elif aniso(new_spacing):
        do_separate_z, axis = True, lowres_axis(new_spacing)
    else:
        do_separate_z, axis = False, None
    if axis is not None:
        if len(axis) in (2, 3):
            do_separate_z, axis = False, None
        else:
            axis = int(axis[0])
    return do_separate_z, axis


def compute_new_shape(old_shape: Sequence[int], old_spacing: Sequence[float], new_spacing: Sequence[float]):
    """preprocessing/resampling/default_resampling.py:25-31 (python ``round``: half to even)."""
    assert len(old_spacing) == len(old_shape) and len(old_shape) == len(new_spacing)
    return [int(round(i / j * k)) for i, j, k in zip(old_spacing, new_spacing, old_shape)]


DEFAULT_RESAMPLING_FN = 'resample_data_or_seg_to_shape'
TORCH_RESAMPLING_FN = 'resample_torch_fornnunet'
NO_RESAMPLING_FNS = ('no_resampling_data_or_seg_to_shape', 'no_resampling_hack')     # upstream's name, the reference's name
_TORCH_KWARGS = ('is_seg', 'num_threads', 'device', 'memefficient_seg_resampling', 'force_separate_z',
                 'separate_z_anisotropy_threshold', 'mode', 'aniso_axis_mode')


def plan_resampling(fn_name: str, kwargs: Optional[dict], current_spacing, new_spacing) -> dict:
    """Which resampling path a configuration's ``resampling_fn_*`` name and kwargs select - the whole decision, without
    a GPU.  -> ``{'path': 'default'}`` (``resample_data_or_seg_to_shape``: the B-spline family, which reads its kwargs
    itself), ``{'path': 'none'}`` (the no-resampling planners: data passes as it is) or, for
    ``resample_torch_fornnunet`` (preprocessing/resampling/resample_torch.py:96-154),
    ``{'path': 'torch', 'separate_axis': None | 0..2, 'memefficient': bool}``.  ``num_threads`` and ``device`` are
    accepted and ignored; ``mode`` other than ``'linear'`` and ``aniso_axis_mode`` other than ``'nearest-exact'`` raise
    NotImplementedError; any other function name raises RuntimeError.

    The reference's separate-z branch cannot run: ``determine_do_sep_z_and_axis`` returns the axis as an integer and
    the branch then calls ``len(axis)`` on it (TypeError).  This builds what the branch states, as upstream nnU-Net
    does with that line fixed: linear in the plane, then nearest-exact along the axis."""
    kwargs = dict(kwargs or {})
    if fn_name == DEFAULT_RESAMPLING_FN:
        return {'path': 'default'}
    if fn_name in NO_RESAMPLING_FNS:
        return {'path': 'none'}
    if fn_name != TORCH_RESAMPLING_FN:
        raise RuntimeError(f"Unable to find resampling function named '{fn_name}': this engine implements "
                           f"{DEFAULT_RESAMPLING_FN}, {TORCH_RESAMPLING_FN} and {NO_RESAMPLING_FNS[0]}")
    unknown = sorted(set(kwargs) - set(_TORCH_KWARGS))
    if unknown:
        raise TypeError(f'{TORCH_RESAMPLING_FN}() got unexpected keyword arguments {unknown}')
    if kwargs.get('mode', 'linear') != 'linear':
        raise NotImplementedError(f"{TORCH_RESAMPLING_FN}: mode={kwargs['mode']!r} (only 'linear' is implemented)")
    if kwargs.get('aniso_axis_mode', 'nearest-exact') != 'nearest-exact':
        raise NotImplementedError(f"{TORCH_RESAMPLING_FN}: aniso_axis_mode={kwargs['aniso_axis_mode']!r} "
                                  f"(only 'nearest-exact' is implemented)")
    do_sep, axis = determine_do_sep_z_and_axis(kwargs.get('force_separate_z', None), current_spacing, new_spacing,
                                               kwargs.get('separate_z_anisotropy_threshold', ANISO_THRESHOLD))
    return {'path': 'torch', 'separate_axis': int(axis) if do_sep else None,
            'memefficient': bool(kwargs.get('memefficient_seg_resampling', False))}


def plan_label_export(fn_name: str, kwargs: Optional[dict], current_spacing, new_spacing, in_shape, out_shape) -> dict:
    """How the labels of a case come out of its logits ``[heads, *in_shape]`` on the grid ``out_shape`` under the
    configuration's ``resampling_fn_probabilities`` - the whole decision, without a GPU.
    -> ``{'path': ..., 'separate_axis': None | 0..2}`` with path

    * ``'same-grid'``: nothing is resampled (equal grids, or a no-resampling planner): the label rule on the logits;
    * ``'fused-default'``: ``resample_data_or_seg_to_shape`` with ``order == 1`` and ``order_z == 0`` (what every standard
      plan asks for probabilities) - ``fnn_resample_labels`` interpolates and picks in one pass;
    * ``'fused-torch'``: ``resample_torch_fornnunet`` - the same entry, the torch family's arithmetic;
    * ``'two-step'``: any other order: the resampled logits are written (``fnn_resample``), then the label rule.

    What ``plan_resampling`` refuses is refused here with the same exception."""
    plan = plan_resampling(fn_name, kwargs, current_spacing, new_spacing)
    if plan['path'] == 'none' or [int(i) for i in in_shape] == [int(i) for i in out_shape]:
        return {'path': 'same-grid', 'separate_axis': None}
    if plan['path'] == 'torch':
        return {'path': 'fused-torch', 'separate_axis': plan['separate_axis']}
    kwargs = dict(kwargs or {})
    do_sep, axis = determine_do_sep_z_and_axis(kwargs.get('force_separate_z', None), current_spacing, new_spacing,
                                               kwargs.get('separate_z_anisotropy_threshold', ANISO_THRESHOLD))
    fused = int(kwargs.get('order', 3)) == 1 and int(kwargs.get('order_z', 0)) == 0
    return {'path': 'fused-default' if fused else 'two-step', 'separate_axis': int(axis) if do_sep else None}


def plan_ensemble_export(member_plans: Sequence[dict]) -> str:
    """How an ensemble's labels come out of its members' logits, from the members' ``plan_label_export`` results - without
    a GPU.  -> ``'fused'``: every member is ``same-grid``, ``fused-default`` or ``fused-torch``, so one
    ``fnn_ensemble_resample_export`` call reads the members' network-grid logits; ``'two-step'`` as soon as one member is
    ``two-step`` (an order other than 1): every member's logits are resampled to the cropped grid first.  (A member whose
    plan ``plan_resampling`` refuses never gets here: ``plan_label_export`` raised.)"""
    member_plans = list(member_plans)
    if not member_plans:
        raise ValueError('an ensemble has at least one member')
    for plan in member_plans:
        if plan['path'] not in ('same-grid', 'fused-default', 'fused-torch', 'two-step'):
            raise ValueError(f"unknown label export path {plan['path']!r}")
    return 'two-step' if any(plan['path'] == 'two-step' for plan in member_plans) else 'fused'


def probabilities_resampling(plans_manager, configuration_manager, properties_dict: dict):
    """What export_prediction.py:26-35 resamples a case's logits with -> (``resampling_fn_probabilities`` name, its kwargs,
    the spacing of the logits, the spacing of the cropped grid), all on the transposed axes."""
    spacing_transposed = [properties_dict['spacing'][i] for i in plans_manager.transpose_forward]
    target = list(configuration_manager.spacing)
    current_spacing = target if len(target) == len(properties_dict['shape_after_cropping_and_before_resampling']) \
        else [spacing_transposed[0], *target]
    kw = getattr(configuration_manager, 'resampling_fn_probabilities_kwargs', None) or \
        {'is_seg': False, 'order': 1, 'order_z': 0, 'force_separate_z': None}
    fn = getattr(configuration_manager, 'resampling_fn_probabilities_name', DEFAULT_RESAMPLING_FN)
    return fn, kw, current_spacing, spacing_transposed


def case_label_export_plan(logits_shape, plans_manager, configuration_manager, properties_dict: dict) -> dict:
    """``plan_label_export`` for logits ``[*logits_shape]`` (the network grid, without the heads) of a preprocessed case."""
    fn, kw, current_spacing, spacing_transposed = probabilities_resampling(plans_manager, configuration_manager, properties_dict)
    return plan_label_export(fn, kw, current_spacing, spacing_transposed, logits_shape,
                             properties_dict['shape_after_cropping_and_before_resampling'])


class DevicePreprocessor:
    def __init__(self, device: torch.device = torch.device('cuda'), verbose: bool = False):
        if device.type != 'cuda':
            raise RuntimeError('DevicePreprocessor has no CPU path: pass a GPU device')
        self.device = device
        self.verbose = verbose
        self._region_orders = {}          # regions_class_order -> its int32 copy on the device (fnn_resample_labels reads it there)

    def _stream(self) -> int:
        return torch.cuda.current_stream(self.device).cuda_stream

    @torch.inference_mode()
    def run_case_npy(self, data: Union[np.ndarray, torch.Tensor], seg, properties: dict, plans_manager,
                     configuration_manager, dataset_json=None) -> Tuple[torch.Tensor, Optional[torch.Tensor], dict]:
        """-> (float32 ``[C, x, y, z]`` on the device, seg, properties) - the ``data`` the predictor consumes.
        ``seg`` (the previous stage's segmentation of a cascade, ``[1, s0, s1, s2]``) travels with the image: transposed,
        cropped to the same box and resampled with ``resampling_fn_seg`` (int16 on the device), so that it stays aligned
        (inference/data_iterators.py:195-201); the -1 the reference writes outside the non-zero mask (cropping.py:36) is
        not produced - it only ever meets ``convert_labelmap_to_one_hot`` over the foreground labels."""
        seg_in = seg
        with torch.cuda.device(self.device):
            raw = torch.as_tensor(data).to(device=self.device, dtype=torch.float32).contiguous()   # :49 astype(float32)
            assert raw.ndim == 4, 'data must have shape (C, X, Y, Z)'
            tf = [int(i) for i in plans_manager.transpose_forward]
            original_spacing = [properties['spacing'][i] for i in tf]
            shape_t = [int(raw.shape[1 + i]) for i in tf]
            properties['shape_before_cropping'] = tuple(shape_t)
            bbox = capi.nonzero_bbox(raw.data_ptr(), raw.shape, tf, self._stream())
            properties['bbox_used_for_cropping'] = bbox
            cropped = [hi - lo for lo, hi in bbox]
            properties['shape_after_cropping_and_before_resampling'] = tuple(cropped)
            target_spacing = list(configuration_manager.spacing)
            if len(target_spacing) < 3:                     # 2d configurations keep the slice spacing (:74-77)
                target_spacing = [original_spacing[0]] + target_spacing
            new_shape = compute_new_shape(cropped, original_spacing, target_spacing)
            schemes = configuration_manager.normalization_schemes
            masks = configuration_manager.use_mask_for_norm
            props = plans_manager.foreground_intensity_properties_per_channel
            norms = []
            for c in range(raw.shape[0]):
                if schemes[c] not in _SCHEMES:
                    raise RuntimeError(f"Unable to locate class '{schemes[c]}' for normalization")
                ip = props.get(str(c), {}) if props else {}
                if schemes[c] == 'CTNormalization':
                    assert ip, 'CTNormalization requires intensity properties'
                    norms.append((_SCHEMES[schemes[c]], ip['mean'], ip['std'], ip['percentile_00_5'], ip['percentile_99_5']))
                else:
                    norms.append((_SCHEMES[schemes[c]], 0., 1., 0., 0., int(bool(masks[c]))))
            out = torch.empty((raw.shape[0], *cropped), dtype=torch.float32, device=self.device)
            capi.preprocess(raw.data_ptr(), raw.shape, tf, bbox, norms, out.data_ptr(), self._stream())
            # normalisation happens before resampling, like the reference (:83-91)
            out = self.resample(out, new_shape, original_spacing, target_spacing,
                                getattr(configuration_manager, 'resampling_fn_data_kwargs', None) or
                                {'is_seg': False, 'order': 3, 'order_z': 0, 'force_separate_z': None},
                                getattr(configuration_manager, 'resampling_fn_data_name', DEFAULT_RESAMPLING_FN))
            seg_out = None
            if seg_in is not None:
                sg = torch.as_tensor(seg_in).to(self.device)
                assert sg.ndim == 4 and tuple(sg.shape[1:]) == tuple(raw.shape[1:]), 'seg must have shape (1, X, Y, Z) of the image'
                sg = sg.permute(0, *[1 + i for i in tf])
                sg = sg[(slice(None), *[slice(lo, hi) for lo, hi in bbox])].to(torch.int16).contiguous()
                seg_out = self.resample_seg(sg, new_shape, original_spacing, target_spacing,
                                            getattr(configuration_manager, 'resampling_fn_seg_kwargs', None) or
                                            {'is_seg': True, 'order': 1, 'order_z': 0, 'force_separate_z': None},
                                            getattr(configuration_manager, 'resampling_fn_seg_name', DEFAULT_RESAMPLING_FN))
        return out, seg_out, properties

    @torch.inference_mode()
    def resample_seg(self, seg: torch.Tensor, new_shape, current_spacing, new_spacing, kwargs: dict,
                     fn_name: str = DEFAULT_RESAMPLING_FN) -> torch.Tensor:
        """``resample_data_or_seg_to_shape(seg, ..., is_seg=True, order, order_z=0)`` (default_resampling.py:113-196)
        with ``resize_segmentation`` (batchgenerators): order 0 resizes the label image; otherwise every label's mask
        is resized (``fnn_resample``, the images' kernel) and the voxels where it reaches 0.5 take the label, labels
        ascending.  Thresholding commutes with the nearest-neighbour pass along an anisotropic axis, so the per-slice
        path is the same call with ``separate_axis``.  ``[C, x, y, z]`` integer tensor -> int16 on the device.
        ``fn_name`` is the configuration's ``resampling_fn_seg`` (``plan_resampling``): ``resample_torch_fornnunet``
        runs ``fnn_resample_torch_seg`` - one pass, the fp16-argmax rule or the ``memefficient_seg_resampling`` one."""
        plan = plan_resampling(fn_name, kwargs, current_spacing, new_spacing)
        if plan['path'] != 'default':
            with torch.cuda.device(self.device):
                sg = seg.to(device=self.device, dtype=torch.int16).contiguous()
                if plan['path'] == 'none' or [int(i) for i in sg.shape[1:]] == [int(i) for i in new_shape]:
                    return sg
                out = torch.empty((sg.shape[0], *[int(i) for i in new_shape]), dtype=torch.int16, device=self.device)
                capi.resample_torch(sg.data_ptr(), sg.shape, new_shape, plan['separate_axis'], False, out.data_ptr(),
                                    self._stream(), is_seg=True, memefficient=plan['memefficient'])
            return out
        if int(kwargs.get('order_z', 0)) != 0:
            raise NotImplementedError('order_z != 0 for segmentations (the reference\'s plans use 0)')
        new_shape = [int(i) for i in new_shape]
        with torch.cuda.device(self.device):
            sg = seg.to(self.device)
            if [int(i) for i in sg.shape[1:]] == new_shape:
                return sg.to(torch.int16)
            order = int(kwargs.get('order', 1))
            kw = dict(kwargs, is_seg=False)
            if order == 0:
                return self.resample(sg.float(), new_shape, current_spacing, new_spacing, kw).round().to(torch.int16)
            out = torch.zeros((sg.shape[0], *new_shape), dtype=torch.int16, device=self.device)
            for c in torch.unique(sg).tolist():                              # ascending, like np.unique
                m = self.resample((sg == c).float(), new_shape, current_spacing, new_spacing, kw)
                out[m >= 0.5] = int(c)
        return out

    @torch.inference_mode()
    def resample(self, data: torch.Tensor, new_shape, current_spacing, new_spacing, kwargs: dict,
                 fn_name: str = DEFAULT_RESAMPLING_FN) -> torch.Tensor:
        """``resample_data_or_seg_to_shape(data, new_shape, current_spacing, new_spacing, **kwargs)`` for images /
        logits (``is_seg`` False): fp32 or fp16 ``[C, x, y, z]`` on the device.  ``fn_name`` is the configuration's
        ``resampling_fn_data`` / ``resampling_fn_probabilities`` (``plan_resampling``): ``resample_torch_fornnunet``
        runs ``fnn_resample_torch`` (one fused linear pass; output dtype = input dtype), the no-resampling name
        returns the data as it is, an unknown name raises."""
        if kwargs.get('is_seg', False):
            raise ValueError('is_seg=True: call resample_seg')
        plan = plan_resampling(fn_name, kwargs, current_spacing, new_spacing)
        if plan['path'] == 'none':
            return data
        if plan['path'] == 'torch':
            with torch.cuda.device(self.device):
                x = data.to(self.device)
                if x.dtype not in (torch.float32, torch.half):
                    x = x.float()
                x = x.contiguous()
                if [int(i) for i in x.shape[1:]] == [int(i) for i in new_shape]:
                    return x
                out = torch.empty((x.shape[0], *[int(i) for i in new_shape]), dtype=x.dtype, device=self.device)
                capi.resample_torch(x.data_ptr(), x.shape, new_shape, plan['separate_axis'], x.dtype == torch.half,
                                    out.data_ptr(), self._stream())
            return out
        do_sep, axis = determine_do_sep_z_and_axis(kwargs.get('force_separate_z', None), current_spacing, new_spacing,
                                                   kwargs.get('separate_z_anisotropy_threshold', ANISO_THRESHOLD))
        with torch.cuda.device(self.device):
            x = data.to(self.device)
            if x.dtype not in (torch.float32, torch.half):
                x = x.float()
            x = x.contiguous()
            out = torch.empty((x.shape[0], *[int(i) for i in new_shape]), dtype=x.dtype, device=self.device)
            capi.resample(x.data_ptr(), x.shape, new_shape, kwargs.get('order', 3), axis if do_sep else None,
                          x.dtype == torch.half, out.data_ptr(), self._stream(), order_z=kwargs.get('order_z', 0))
        return out

    @torch.inference_mode()
    def convert_predicted_logits_to_segmentation_with_correct_shape(self, predicted_logits: torch.Tensor, predictor,
                                                                    plans_manager, configuration_manager,
                                                                    properties_dict: dict) -> torch.Tensor:
        """inference/export_prediction.py:16-53 on the device: logits ``[heads, x, y, z]`` of the network grid ->
        label map on the original image grid.  ``predictor`` supplies the label rule (its ``label_manager``)."""
        fn, kw, current_spacing, spacing_transposed = probabilities_resampling(plans_manager, configuration_manager,
                                                                               properties_dict)
        cropped = properties_dict['shape_after_cropping_and_before_resampling']
        if getattr(predictor, 'fused_label_export', False):
            # no resampled logits [heads, *cropped] in between: interpolation and label rule in one pass
            plan = plan_label_export(fn, kw, current_spacing, spacing_transposed, predicted_logits.shape[1:], cropped)
            if plan['path'] in ('fused-default', 'fused-torch'):
                order, u16 = label_rule(predictor.label_manager)
                seg = self.resample_logits_to_labels(predicted_logits, cropped, plan['path'] == 'fused-torch',
                                                     plan['separate_axis'], order, u16)
                return self.revert_labels(seg, properties_dict, plans_manager, predictor.label_manager)
        logits = self.resample(predicted_logits, cropped, current_spacing, spacing_transposed, kw, fn)
        seg = predictor.convert_logits_to_segmentation(logits)
        return self.revert_labels(seg, properties_dict, plans_manager, predictor.label_manager)

    @torch.inference_mode()
    def resample_logits_to_labels(self, logits: torch.Tensor, new_shape, torch_family: bool, separate_axis,
                                  regions_class_order, u16: bool) -> torch.Tensor:
        """``fnn_resample_labels``: logits ``[heads, x, y, z]`` (fp16 / fp32) -> the labels of the logits resampled to
        ``new_shape`` (default family at order 1, or the torch family), bit for bit those of ``resample`` followed by the
        label rule, without the resampled tensor.  ``regions_class_order`` None is the argmax rule.  -> uint8, or the
        int32-carried uint16 (``u16``) of the predictor, on the device."""
        new_shape = [int(i) for i in new_shape]
        with torch.cuda.device(self.device):
            lg = logits.to(self.device)
            if lg.dtype not in (torch.half, torch.float32):
                lg = lg.float()
            lg = lg.contiguous()
            order_ptr = None
            if regions_class_order is not None:
                key = tuple(int(c) for c in regions_class_order)
                if key not in self._region_orders:
                    self._region_orders[key] = torch.tensor(key, dtype=torch.int32, device=self.device)
                order_ptr = self._region_orders[key].data_ptr()
            labels = torch.empty(new_shape, dtype=torch.int16 if u16 else torch.uint8, device=self.device)
            capi.resample_labels(lg.data_ptr(), lg.dtype == torch.half, lg.shape, new_shape,
                                 capi.FNN_RESAMPLE_TORCH if torch_family else capi.FNN_RESAMPLE_DEFAULT, separate_axis,
                                 order_ptr, lg.shape[0], labels.data_ptr(), u16, self._stream())
        return as_plain_labels(labels)

    @torch.inference_mode()
    def resample_logits_to_cropped_shape(self, predicted_logits: torch.Tensor, plans_manager, configuration_manager,
                                         properties_dict: dict) -> torch.Tensor:
        """The resampling step of export_prediction.py:26-35: logits of the network grid ->
        ``shape_after_cropping_and_before_resampling`` (returned as they are when the grids agree)."""
        fn, kw, current_spacing, spacing_transposed = probabilities_resampling(plans_manager, configuration_manager,
                                                                               properties_dict)
        cropped = [int(i) for i in properties_dict['shape_after_cropping_and_before_resampling']]
        logits = predicted_logits
        if [int(i) for i in logits.shape[1:]] != cropped:
            logits = self.resample(logits, cropped, current_spacing, spacing_transposed, kw, fn)
        return logits

    @torch.inference_mode()
    def convert_predicted_logits_to_segmentation_and_probabilities(self, predicted_logits: torch.Tensor, predictor,
                                                                   plans_manager, configuration_manager,
                                                                   properties_dict: dict) -> Tuple[torch.Tensor, torch.Tensor]:
        """export_prediction.py:16-70 with ``return_probabilities=True``: -> (label map, float32 probabilities
        ``[heads, s0, s1, s2]``), both on the original image grid, both on the device."""
        logits = self.resample_logits_to_cropped_shape(predicted_logits, plans_manager, configuration_manager,
                                                       properties_dict)
        order, u16 = label_rule(predictor.label_manager)
        with torch.cuda.device(self.device):
            lg = logits.to(self.device)
            if lg.dtype not in (torch.half, torch.float32):
                lg = lg.float()
            lg = lg.contiguous()
            before = [int(i) for i in properties_dict['shape_before_cropping']]
            tb = [int(i) for i in plans_manager.transpose_backward]
            grid = [before[j] for j in tb]
            probs = torch.empty((lg.shape[0], *grid), dtype=torch.float32, device=self.device)
            labels = torch.empty(grid, dtype=torch.int16 if u16 else torch.uint8, device=self.device)
            capi.export_probabilities(lg.data_ptr(), lg.dtype == torch.half, lg.shape[0], order,
                                      properties_dict['bbox_used_for_cropping'], before, tb, probs.data_ptr(),
                                      labels.data_ptr(), u16, self._stream())
        return as_plain_labels(labels), probs

    @torch.inference_mode()
    def revert_labels(self, segmentation: torch.Tensor, properties: dict, plans_manager, label_manager) -> torch.Tensor:
        """Cropped label map (uint8, or the int32-carried uint16 of the predictor) -> the original image grid."""
        u16 = len(label_manager.foreground_labels) >= 255                      # export_prediction.py:45-46
        with torch.cuda.device(self.device):
            seg = segmentation.to(self.device)
            seg = (seg.to(torch.int16) if u16 else seg.to(torch.uint8)).contiguous()
            before = [int(i) for i in properties['shape_before_cropping']]
            tb = [int(i) for i in plans_manager.transpose_backward]
            out = torch.empty([before[j] for j in tb], dtype=seg.dtype, device=self.device)
            capi.revert_labels(seg.data_ptr(), u16, properties['bbox_used_for_cropping'], before, tb, out.data_ptr(),
                               self._stream())
        return as_plain_labels(out)
