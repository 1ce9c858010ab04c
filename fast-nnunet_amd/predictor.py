"""Drop-in ``nnUNetPredictor`` backed by the MI355X HIP engine.

Mirrors the public surface of the reference's
``nnunetv2.inference.predict_from_raw_data.nnUNetPredictor``
(distillation/nnunetv2/inference/predict_from_raw_data.py:39-680) for the hot
path: constructor knobs, ``initialize_from_trained_model_folder``,
``manual_initialization``, ``predict_sliding_window_return_logits``,
``predict_logits_from_preprocessed_data`` and the attributes callers read
(``network``, ``plans_manager``, ``configuration_manager``, ``label_manager``,
``dataset_json``, ``list_of_parameters``, ``allowed_mirroring_axes``,
``device``, ``verbose``).  Everything numerical happens in
``csrc/libfnn_hip.so``; torch is only used for device memory and streams.

There is no CPU path: the predictor raises if the HIP library or a GPU is
missing.
"""
from __future__ import annotations

import itertools
import os
from copy import deepcopy
from typing import List, Optional, Tuple, Union

import numpy as np
import torch

from . import capi
from .arch import ArchSpec, check_against_plans, ops_from_plans, spec_from_state_dict, weight_blob
from .case_pipeline import as_plain_labels, compress_mode, device_compressor, export_case_files, labels_for_writer, run_pipeline
from .label_folders import load_json
from .plans import ConfigurationManager, PlansManager, determine_num_input_channels, label_rule
from .sliding_window import compute_gaussian, compute_steps_for_sliding_window


class nnUNetPredictor(object):
    def __init__(self,
                 tile_step_size: float = 0.5,
                 use_gaussian: bool = True,
                 use_mirroring: bool = True,
                 perform_everything_on_device: bool = True,
                 device: torch.device = torch.device('cuda'),
                 verbose: bool = False,
                 verbose_preprocessing: bool = False,
                 allow_tqdm: bool = True,
                 accumulate_in: str = 'fp16',
                 patches_per_forward: int = 4,
                 compute_dtype: str = 'f16',
                 fused_label_export: bool = True,
                 compress_on_device: Union[bool, str] = False):
        """Same knobs as the reference (:40-65) plus the engine's choices:

        accumulate_in  'fp16' reproduces the reference's half accumulators and their rounding per patch visit as the
                       reference computes them WITHOUT autocast (its CPU path: fp32 logits and products, one rounding
                       per visit); 'fp16_autocast' as it computes them on a GPU (:591-593 - the network returns fp16,
                       so the logit, the mirror sums, the Gaussian product and the sum are each rounded to fp16);
                       'fp32' is the exact blend.
        patches_per_forward  how many patches one network forward batches.
        compute_dtype  'f16' (default: the mode every parity statement is for) or 'f8': OCP e4m3 operands in
                       the 3x3x3 stride-1 convolutions (BASELINE config 5; budget in DESIGN.md).
        fused_label_export  a case whose logits are resampled back (file spacing != target spacing) gets its labels from
                       ``fnn_resample_labels`` - interpolation and label rule in one pass, no resampled logits in memory
                       (order-1 default plans and torch-resampling plans); False: resample, then the label rule - the
                       same labels.
        compress_on_device  labels bound for a ``.nii.gz`` file are compressed by ``fnn_deflate_labels`` on the GPU and
                       only the compressed bytes are downloaded; the file holds the same header and voxels behind another
                       (larger, valid) deflate stream.  False (default): the host's gzip, byte for byte as before.
                       Returned arrays, ``.npz`` and ``.pkl`` are the same either way.  ``'dynamic'``: the same route
                       with per-chunk dynamic Huffman tables (``fnn_deflate_labels_dyn``) - smaller files, which
                       ``NiftiIO(inflate_on_device='dynamic')`` inflates on the GPU (``inflate_on_device=True`` reads them
                       through its zlib fallback).  Anything but False, True
                       and ``'dynamic'`` is a ValueError.
        """
        self.verbose = verbose
        self.verbose_preprocessing = verbose_preprocessing
        self.allow_tqdm = allow_tqdm
        self.plans_manager, self.configuration_manager, self.list_of_parameters, self.network, self.dataset_json, \
            self.trainer_name, self.allowed_mirroring_axes, self.label_manager = (None,) * 8
        self.tile_step_size = tile_step_size
        self.use_gaussian = use_gaussian
        self.use_mirroring = use_mirroring
        device = torch.device(device)
        if device.type != 'cuda':
            raise RuntimeError('this predictor runs on an AMD GPU through the HIP engine; there is no CPU path '
                               f'(got device={device}). Use the reference predictor for CPU inference.')
        self.device = device
        self.perform_everything_on_device = perform_everything_on_device
        if accumulate_in not in ('fp16', 'fp32', 'fp16_autocast'):
            raise ValueError("accumulate_in must be 'fp16', 'fp32' or 'fp16_autocast'")
        self.accumulate_in = accumulate_in
        self.patches_per_forward = int(patches_per_forward)
        if compute_dtype not in ('f16', 'f8'):
            raise ValueError("compute_dtype must be 'f16' or 'f8'")
        self.compute_dtype = compute_dtype
        self.fused_label_export = bool(fused_label_export)
        self.compress_on_device = compress_mode(compress_on_device)
        self._engine: Optional[capi.Engine] = None
        self._spec: Optional[ArchSpec] = None
        self._active_fold = 0
        self._postprocessing = None
        self._rw = None

    # ------------------------------------------------------------------ init
    def initialize_from_trained_model_folder(self, model_training_output_dir: str,
                                             use_folds: Union[Tuple[Union[int, str]], None],
                                             checkpoint_name: str = 'checkpoint_final.pth'):
        """Model folder -> plans, dataset.json, per-fold weights (:67-129)."""
        if use_folds is None:
            use_folds = nnUNetPredictor.auto_detect_available_folds(model_training_output_dir, checkpoint_name)
        dataset_json = load_json(os.path.join(model_training_output_dir, 'dataset.json'))
        plans_manager = PlansManager(load_json(os.path.join(model_training_output_dir, 'plans.json')))
        if isinstance(use_folds, (str, int)):
            use_folds = [use_folds]
        parameters, trainer_name, configuration_name, mirror_axes, init_args = [], None, None, None, {}
        for i, f in enumerate(use_folds):
            f = int(f) if f != 'all' else f
            checkpoint = torch.load(os.path.join(model_training_output_dir, f'fold_{f}', checkpoint_name),
                                    map_location=torch.device('cpu'), weights_only=False)
            if i == 0:
                trainer_name = checkpoint['trainer_name']
                init_args = checkpoint.get('init_args', {})
                configuration_name = init_args['configuration']
                mirror_axes = checkpoint.get('inference_allowed_mirroring_axes')
            parameters.append(checkpoint['network_weights'])
        configuration_manager = plans_manager.get_configuration(configuration_name)
        self.plans_manager = plans_manager
        self.configuration_manager = configuration_manager
        self.list_of_parameters = parameters
        self.dataset_json = dataset_json
        self.trainer_name = trainer_name
        self.allowed_mirroring_axes = mirror_axes
        self.label_manager = plans_manager.get_label_manager(dataset_json)
        self.network = None
        self._reduction = init_args.get('feature_reduction_factor')
        self._configuration_name = configuration_name
        self._build_engine()

    def manual_initialization(self, network, plans_manager: PlansManager,
                              configuration_manager: ConfigurationManager, parameters: Optional[List[dict]],
                              dataset_json: dict, trainer_name: str,
                              inference_allowed_mirroring_axes: Optional[Tuple[int, ...]]):
        """In-process initialisation (:131-154).  ``network`` may be the torch module the caller built
        (its state dict is read when ``parameters`` is None) or None when ``parameters`` are given."""
        self.plans_manager = plans_manager
        self.configuration_manager = configuration_manager
        self.list_of_parameters = parameters
        self.network = network
        self.dataset_json = dataset_json
        self.trainer_name = trainer_name
        self.allowed_mirroring_axes = inference_allowed_mirroring_axes
        self.label_manager = plans_manager.get_label_manager(dataset_json)
        self._reduction = None
        self._build_engine()

    def set_postprocessing(self, postprocessing):
        """Connected-component postprocessing for ``predict_single_npy_array`` (not in the reference's predictor, which
        leaves it to ``nnUNetv2_apply_postprocessing``): the path of a ``postprocessing.pkl``, a ``(pp_fns,
        pp_fn_kwargs)`` pair as that file holds, or None (the default: no postprocessing).  The steps run on the device
        label map on the raw grid, before it is copied to the host; probabilities are never changed."""
        from .postprocessing import load_postprocessing_pkl
        if postprocessing is None:
            self._postprocessing = None
        elif isinstance(postprocessing, (str, os.PathLike)):
            self._postprocessing = load_postprocessing_pkl(postprocessing)
        else:
            pp_fns, pp_fn_kwargs = postprocessing
            if len(pp_fns) != len(pp_fn_kwargs):
                raise ValueError('postprocessing: as many kwargs as functions expected')
            self._postprocessing = (list(pp_fns), [dict(k) for k in pp_fn_kwargs])

    def _labels_out(self, labels: torch.Tensor, props: dict, for_file: bool):
        """The labels of a case as they leave the device: postprocessed (in the frame of the image as it was read), then
        ``labels_for_writer`` in the label manager's width - the host array, or when they are bound for a file whatever the
        reader-writer's ``write_seg`` takes without a GPU call (``_label_files`` says whether that is compressed here)."""
        if self._postprocessing is not None:
            from .postprocessing import apply_postprocessing
            labels = apply_postprocessing(labels, *self._postprocessing)
        rw = self._reader_writer() if for_file else None
        return labels_for_writer(rw, labels, props, label_rule(self.label_manager)[1],
                                 self._label_files(rw)[0] if for_file else None)

    @staticmethod
    def auto_detect_available_folds(model_training_output_dir, checkpoint_name):
        print('use_folds is None, attempting to auto detect available folds')
        found = []
        for name in sorted(os.listdir(model_training_output_dir)):
            full = os.path.join(model_training_output_dir, name)
            if os.path.isdir(full) and name.startswith('fold_') and name != 'fold_all' \
                    and os.path.isfile(os.path.join(full, checkpoint_name)):
                found.append(int(name.split('_')[-1]))
        print(f'found the following folds: {found}')
        return found

    def _state_dicts(self) -> List[dict]:
        if self.list_of_parameters:
            return list(self.list_of_parameters)
        if self.network is not None and hasattr(self.network, 'state_dict'):
            return [self.network.state_dict()]
        raise RuntimeError('no parameters: pass `parameters` or a network with a state_dict')

    def _build_engine(self):
        sds = self._state_dicts()
        patch = tuple(self.configuration_manager.patch_size)
        if len(patch) not in (2, 3):
            raise NotImplementedError('patch_size must have two (2d) or three (3d_fullres / 3d_lowres) entries')
        kw = {}
        try:
            kw = self.configuration_manager.network_arch_init_kwargs or {}
        except (KeyError, TypeError):
            kw = {}
        eps, slope = ops_from_plans(kw) if kw else (1e-5, 0.01)
        spec = spec_from_state_dict(sds[0], patch, eps=eps, slope=slope)
        if kw and 'n_stages' in kw and 'strides' in kw:
            check_against_plans(spec, kw, self._reduction)
        spec.precision = capi.FNN_PREC_F8 if self.compute_dtype == 'f8' else capi.FNN_PREC_F16
        heads = self.label_manager.num_segmentation_heads
        if heads != spec.num_heads:
            raise RuntimeError(f'checkpoint has {spec.num_heads} segmentation heads, dataset.json implies {heads}')
        if self._engine is not None:
            self._engine.close()
        idx = self.device.index if self.device.index is not None else torch.cuda.current_device()
        self._engine = capi.Engine(spec.to_desc(), device=idx, max_batch=max(1, self.patches_per_forward))
        for f, sd in enumerate(sds):
            blob = weight_blob(spec, sd)
            if blob.size != self._engine.weight_count:
                raise RuntimeError('internal error: weight blob size mismatch')
            self._engine.load_weights(f, blob)
        g = compute_gaussian(patch, sigma_scale=1. / 8, value_scaling_factor=10, device=torch.device('cpu'))
        self._engine.set_gaussian(g.contiguous().view(torch.int16).numpy().view(np.uint16))
        self._spec = spec
        self._rw = None
        self._n_folds = len(sds)
        self._active_fold = 0

    # --------------------------------------------------------------- predict
    def _opts(self) -> capi.Opts:
        o = capi.Opts()
        o.tile_step_size = float(self.tile_step_size)
        o.use_gaussian = int(bool(self.use_gaussian))
        axes = self.allowed_mirroring_axes if self.use_mirroring else None
        if axes is not None:
            nd = self._spec.spatial_dims
            assert max(axes) <= nd - 1, 'mirror_axes does not match the dimension of the input!'
            o.n_mirror_axes = len(axes)
            for i, a in enumerate(axes):
                o.mirror_axes[i] = int(a) + (3 - nd)           # 2-D network axes (y, z) are engine axes 1, 2
        o.accum = {'fp16': capi.FNN_ACC_FP16_REFERENCE, 'fp32': capi.FNN_ACC_FP32, 'fp16_autocast': capi.FNN_ACC_FP16_AUTOCAST}[self.accumulate_in]
        o.out_dtype = capi.FNN_OUT_F16
        o.batch = self.patches_per_forward
        o.stream = torch.cuda.current_stream(self.device).cuda_stream
        return o

    def _internal_get_sliding_window_slicers(self, image_size: Tuple[int, ...]):
        """Patch windows in visit order (:506-538, both branches)."""
        patch = self.configuration_manager.patch_size
        if len(patch) < len(image_size):
            assert len(patch) == len(image_size) - 1, 'if tile_size has less entries than image_size, len(tile_size) ' \
                                                      'must be one shorter than len(image_size)'
            steps = compute_steps_for_sliding_window(image_size[1:], patch, self.tile_step_size)
            return [tuple([slice(None), d, *[slice(s, s + p) for s, p in zip(st, patch)]])
                    for d in range(image_size[0]) for st in itertools.product(*steps)]
        steps = compute_steps_for_sliding_window(image_size, patch, self.tile_step_size)
        return [tuple([slice(None), *[slice(s, s + p) for s, p in zip(st, patch)]])
                for st in itertools.product(*steps)]

    def _resident_or_host(self, t: torch.Tensor) -> torch.Tensor:
        """float32, contiguous.  A CPU tensor (what the reference's callers hold: the preprocessing iterator's output,
        data_iterators.py:116-117; moved with `data.to(results_device)` at :579) STAYS on the CPU: the engine uploads it by
        tiles (planes x rows) on a copy stream and starts a batch when the tiles under its patches have landed (pin the tensor
        for a DMA straight from it; a pageable one goes through the engine's pinned staging ring)."""
        if t.device.type == 'cpu':
            return t.to(dtype=torch.float32).contiguous()
        return t.to(device=self.device, dtype=torch.float32).contiguous()

    def _check_input(self, input_image):
        assert isinstance(input_image, torch.Tensor)
        assert input_image.ndim == 4, 'input_image must be a 4D np.ndarray or torch.Tensor (c, x, y, z)'
        if self._engine is None:
            raise RuntimeError('predictor is not initialised')

    @torch.inference_mode()
    def predict_sliding_window_return_logits(self, input_image: torch.Tensor) -> torch.Tensor:
        """[C,X,Y,Z] preprocessed image -> fp16 logits [heads,X,Y,Z] (:634-680)."""
        self._check_input(input_image)
        with torch.cuda.device(self.device):
            x = self._resident_or_host(input_image)
            out = torch.empty((self._spec.num_heads, *x.shape[1:]), dtype=torch.half, device=self.device)
            self._engine.predict_volume(x.data_ptr(), x.shape, self._opts(), out.data_ptr(), fold=self._active_fold)
        return out if self.perform_everything_on_device else out.cpu()

    @torch.inference_mode()
    def predict_logits_from_preprocessed_data(self, data: torch.Tensor, on_device: bool = False) -> torch.Tensor:
        """Mean over the folds; returned on the CPU like the reference (:471-504) unless ``on_device`` (not in the
        reference: skips its 15 GiB device-to-host copy of a 61-class 512^3 volume)."""
        self._check_input(data)
        with torch.cuda.device(self.device):
            x = self._resident_or_host(data)
            out = torch.empty((self._spec.num_heads, *x.shape[1:]), dtype=torch.half, device=self.device)
            self._engine.predict_volume(x.data_ptr(), x.shape, self._opts(), out.data_ptr(), n_folds=self._n_folds)
        if self.verbose:
            print('Prediction done')
        return out if on_device else out.to('cpu')

    @torch.inference_mode()
    def predict_single_npy_array(self, input_image: np.ndarray, image_properties: dict,
                                 segmentation_previous_stage: np.ndarray = None,
                                 output_file_truncated: str = None,
                                 save_or_return_probabilities: bool = False):
        """Raw image ``[C, s0, s1, s2]`` + ``{'spacing': ...}`` -> label map on the raw grid (numpy, uint8 / uint16) -
        predict_from_raw_data.py:423-468 with every step on the device: ``DevicePreprocessor.run_case_npy``
        (transpose, crop, normalise, resample), the sliding window, then
        ``convert_predicted_logits_to_segmentation_with_correct_shape`` (export_prediction.py:16-53).  When the case
        needs no resampling the labels are taken straight from the accumulators (no logits are materialised).
        ``save_or_return_probabilities=True`` returns ``(labels, float32 probabilities [heads, s0, s1, s2])`` like the
        reference (softmax / sigmoid, background probability 1 outside the crop box).  With ``output_file_truncated`` the
        result is written instead (``<truncated><file_ending>``, and with probabilities ``.npz`` and ``.pkl``) and None
        is returned."""
        seg, probs, props = self._predict_case(input_image, image_properties, segmentation_previous_stage,
                                               save_or_return_probabilities, for_file=output_file_truncated is not None)
        if output_file_truncated is not None:
            # export_prediction_from_logits (export_prediction.py:74-110): <truncated><file_ending> through the plans'
            # reader-writer, with probabilities also <truncated>.npz and the properties as <truncated>.pkl; returns None
            self._export_case(seg, probs, props, output_file_truncated)
            return None
        return (seg, probs) if save_or_return_probabilities else seg

    def _predict_case(self, input_image, image_properties: dict, segmentation_previous_stage=None,
                      save_or_return_probabilities: bool = False, for_file: bool = False):
        """-> (labels on the raw grid (numpy), float32 probabilities or None, the case's properties after preprocessing).
        ``input_image`` is a numpy array or a tensor (a resident one stays where it is).  ``for_file``: the labels go to
        the reader-writer's ``write_seg`` (``_labels_out``); the probabilities stay in the frame of ``input_image``."""
        pp, data, props = self._preprocess_case(input_image, image_properties, segmentation_previous_stage)
        if self.verbose:
            print('predicting')
        same_grid = tuple(data.shape[1:]) == tuple(props['shape_after_cropping_and_before_resampling'])
        if same_grid and not save_or_return_probabilities:
            seg = self.predict_segmentation_from_preprocessed_data(data)
            out = pp.revert_labels(seg, props, self.plans_manager, self.label_manager)
            return self._labels_out(out, props, for_file), None, props
        logits = self._predict_case_logits(data)
        if self.verbose:
            print('resampling to original shape')
        if save_or_return_probabilities:
            out, probs = pp.convert_predicted_logits_to_segmentation_and_probabilities(
                logits, self, self.plans_manager, self.configuration_manager, props)
            return self._labels_out(out, props, for_file), probs.cpu().numpy(), props
        out = pp.convert_predicted_logits_to_segmentation_with_correct_shape(logits, self, self.plans_manager,
                                                                             self.configuration_manager, props)
        return self._labels_out(out, props, for_file), None, props

    def _preprocess_case(self, input_image: np.ndarray, image_properties: dict, segmentation_previous_stage=None):
        """-> (DevicePreprocessor, network input on the device, properties) for predict_single_npy_array."""
        from .preprocess import DevicePreprocessor
        pp = DevicePreprocessor(self.device, verbose=self.verbose)
        props = dict(image_properties)
        if self.verbose:
            print('preprocessing')
        data, seg, props = pp.run_case_npy(input_image, segmentation_previous_stage, props, self.plans_manager,
                                           self.configuration_manager, self.dataset_json)
        if segmentation_previous_stage is not None:
            # cascade: the previous stage's labels as one-hot channels behind the image (convert_labelmap_to_one_hot,
            # label_handling.py:259-292; data_iterators.py:202-204) - the network was built with that many inputs
            # (determine_num_input_channels, label_handling.py:305-310)
            fg = torch.as_tensor(list(self.label_manager.foreground_labels), device=seg.device, dtype=seg.dtype)
            onehot = (seg[0][None] == fg.view(-1, 1, 1, 1)).to(data.dtype)
            data = torch.cat((data, onehot), 0).contiguous()
            if data.shape[0] != self._spec.in_channels:
                raise RuntimeError(f'cascade input has {data.shape[0]} channels (image + {len(fg)} foreground labels), '
                                   f'the network expects {self._spec.in_channels}')
        return pp, data, props

    def _predict_case_logits(self, data: torch.Tensor) -> torch.Tensor:
        """fp16 logits [heads, *network grid] on the device, the mean over the folds."""
        self._check_input(data)
        with torch.cuda.device(self.device):
            logits = torch.empty((self._spec.num_heads, *data.shape[1:]), dtype=torch.half, device=self.device)
            self._engine.predict_volume(data.data_ptr(), data.shape, self._opts(), logits.data_ptr(), n_folds=self._n_folds)
        return logits

    def predict_segmentation_from_preprocessed_data(self, data: torch.Tensor) -> torch.Tensor:
        """Label map on the device, skipping the full-logit D2H copy the reference pays at :386 before
        ``convert_logits_to_segmentation`` (label_handling.py:144-195): argmax for plain labels, sigmoid > 0.5
        painted in ``regions_class_order`` for region-based training; uint8, or uint16 (returned as int32 - torch
        has no uint16 arithmetic) when the dataset has >= 255 foreground labels (export_prediction.py:45-46).
        With one fold the labels are taken straight from the accumulators; the logits are never written."""
        self._check_input(data)
        order, u16 = label_rule(self.label_manager)
        with torch.cuda.device(self.device):
            x = self._resident_or_host(data)
            self._engine.set_label_rule(order, uint16=u16)
            labels = torch.empty(x.shape[1:], dtype=torch.int16 if u16 else torch.uint8, device=self.device)
            self._engine.predict_labels(x.data_ptr(), x.shape, self._opts(), labels.data_ptr(), n_folds=self._n_folds)
        return as_plain_labels(labels)

    def convert_logits_to_segmentation(self, predicted_logits: torch.Tensor) -> torch.Tensor:
        """``LabelManager.convert_logits_to_segmentation`` (label_handling.py:183-195) on resident logits
        ``[heads, X, Y, Z]`` (fp16 or fp32, on the device)."""
        from . import capi
        assert predicted_logits.ndim == 4 and predicted_logits.shape[0] == self._spec.num_heads
        order, u16 = label_rule(self.label_manager)
        with torch.cuda.device(self.device):
            lg = predicted_logits.to(self.device)
            if lg.dtype not in (torch.half, torch.float32):
                lg = lg.float()
            lg = lg.contiguous()
            self._engine.set_label_rule(order, uint16=u16)
            labels = torch.empty(lg.shape[1:], dtype=torch.int16 if u16 else torch.uint8, device=self.device)
            self._engine.argmax_labels(lg.data_ptr(), capi.FNN_OUT_F32 if lg.dtype == torch.float32 else capi.FNN_OUT_F16,
                                       lg.shape[0], lg[0].numel(), labels.data_ptr(),
                                       torch.cuda.current_stream(self.device).cuda_stream)
        return as_plain_labels(labels)

    @torch.inference_mode()
    def forward_patches(self, x: torch.Tensor) -> torch.Tensor:
        """``self.network(x)`` for a batch of patches: [n,C,px,py,pz] -> fp32 logits [n,heads,px,py,pz]
        ([n,C,py,pz] -> [n,heads,py,pz] for a 2-D configuration)."""
        two_d = self._spec.spatial_dims == 2
        sp = tuple(self._spec.patch[1:]) if two_d else tuple(self._spec.patch)
        assert x.ndim == len(sp) + 2 and tuple(x.shape[2:]) == sp
        with torch.cuda.device(self.device):
            xd = x.to(device=self.device, dtype=torch.float32).contiguous()
            out = torch.empty((x.shape[0], self._spec.num_heads, *x.shape[2:]), dtype=torch.float32, device=self.device)
            self._engine.forward_patches(xd.data_ptr(), x.shape[0], out.data_ptr(), fold=self._active_fold,
                                         stream=torch.cuda.current_stream(self.device).cuda_stream)
        return out

    # ----------------------------------------------------------------- files
    def _reader_writer(self):
        """The plans' ``image_reader_writer`` class (``PlansManager.image_reader_writer_class``), or - for plans that do
        not name one - the class the dataset's file ending selects, and ``NiftiReorientIO`` where either names
        ``NibabelIOWithReorient`` (``imageio.prediction_reader_writer_class``); one instance per predictor (it owns pinned
        staging)."""
        if self._rw is None:
            from .imageio import prediction_reader_writer_class
            self._rw = prediction_reader_writer_class(self.plans_manager, self.dataset_json)(self.device)
        return self._rw

    def _label_files(self, rw):
        """The label file(s) of a case, here the one label map (a subclass makes others) -> ``(compress, write)``: what
        compresses the device labels on the calling thread (``labels_for_writer``'s ``compress``; None: they are not), and
        the host-only ``write(seg, props, output_file_truncated)`` that takes what ``_labels_out`` made."""
        ending = self.dataset_json['file_ending']
        return (device_compressor(rw, self.compress_on_device, ending),
                lambda seg, props, truncated: rw.write_seg(seg, truncated + ending, props))

    def _export_case(self, seg, probs, props, output_file_truncated):
        """Host only (numpy, zlib, file writes) once the reader-writer exists: what the writer thread of
        ``predict_from_files`` runs."""
        write = self._label_files(self._reader_writer())[1]
        export_case_files(output_file_truncated, probs, props, lambda: write(seg, props, output_file_truncated))

    def _manage_input_and_output_lists(self, list_of_lists_or_source_folder: Union[str, List[List[str]]],
                                       output_folder_or_list_of_truncated_output_files: Union[None, str, List[str]],
                                       folder_with_segs_from_prev_stage: str = None, overwrite: bool = True,
                                       part_id: int = 0, num_parts: int = 1, save_probabilities: bool = False):
        """predict_from_raw_data.py:166-205: the cases of this part, their truncated output names and previous-stage
        files; with ``overwrite=False`` the cases whose output exists (label file, and ``.npz`` when probabilities are
        asked for) are dropped."""
        ending = self.dataset_json['file_ending']
        if isinstance(list_of_lists_or_source_folder, str):
            list_of_lists_or_source_folder = create_lists_from_splitted_dataset_folder(list_of_lists_or_source_folder, ending)
        print(f'There are {len(list_of_lists_or_source_folder)} cases in the source folder')
        cases = list_of_lists_or_source_folder[part_id::num_parts]
        caseids = [os.path.basename(i[0])[:-(len(ending) + 5)] for i in cases]
        print(f'I am processing {part_id} out of {num_parts} (max process ID is {num_parts - 1}, we start counting with 0!)')
        print(f'There are {len(caseids)} cases that I would like to predict')
        if isinstance(output_folder_or_list_of_truncated_output_files, str):
            truncated = [os.path.join(output_folder_or_list_of_truncated_output_files, i) for i in caseids]
        elif isinstance(output_folder_or_list_of_truncated_output_files, list):
            truncated = output_folder_or_list_of_truncated_output_files[part_id::num_parts]
        else:
            truncated = None
        prev = [os.path.join(folder_with_segs_from_prev_stage, i + ending) if folder_with_segs_from_prev_stage is not None
                else None for i in caseids]
        if not overwrite and truncated is not None:
            done = [os.path.isfile(i + ending) for i in truncated]
            if save_probabilities:
                done = [i and os.path.isfile(j + '.npz') for i, j in zip(done, truncated)]
            todo = [i for i, j in enumerate(done) if not j]
            truncated = [truncated[i] for i in todo]
            cases = [cases[i] for i in todo]
            prev = [prev[i] for i in todo]
            print(f'overwrite was set to {overwrite}, so I am only working on cases that haven\'t been predicted yet. '
                  f'That\'s {len(todo)} cases.')
        return cases, truncated, prev

    def _assert_prev_stage_folder(self, folder_prev):
        """The reference's cascade assertion (predict_from_raw_data.py:232-236)."""
        if self.configuration_manager.previous_stage_name is not None:
            assert folder_prev is not None, \
                f'The requested configuration is a cascaded network. It requires the segmentations of the previous ' \
                f'stage ({self.configuration_manager.previous_stage_name}) as input. Please provide the folder where' \
                f' they are located via folder_with_segs_from_prev_stage'

    def _prepare_files_run(self, call_kwargs: dict, sequential: bool):
        """What both file entry points do before the first case (predict_from_raw_data.py:221-261 / :691-730): the output
        folder with the call's arguments, dataset.json and plans.json; the cascade assertion; the lists."""
        import json
        target = call_kwargs['output_folder_or_list_of_truncated_output_files']
        if isinstance(target, str):
            output_folder = target
        elif isinstance(target, list):
            output_folder = os.path.dirname(target[0]) if target else None
            if output_folder is not None and len(output_folder) == 0:
                output_folder = os.path.curdir
        else:
            output_folder = None
        if output_folder is not None:
            os.makedirs(output_folder, exist_ok=True)
            for name, obj, sort in (('predict_from_raw_data_args.json', deepcopy(call_kwargs), True),
                                    ('dataset.json', self.dataset_json, False), ('plans.json', self.plans_manager.plans, False)):
                with open(os.path.join(output_folder, name), 'w') as f:
                    json.dump(obj, f, indent=4, sort_keys=sort)
        folder_prev = call_kwargs.get('folder_with_segs_from_prev_stage')
        self._assert_prev_stage_folder(folder_prev)
        return self._manage_input_and_output_lists(
            call_kwargs['list_of_lists_or_source_folder'], target, folder_prev, call_kwargs['overwrite'],
            0 if sequential else call_kwargs['part_id'], 1 if sequential else call_kwargs['num_parts'],
            call_kwargs['save_probabilities'])

    def _run_staged_case(self, rw, staged, staged_prev, save_probabilities: bool, for_file: bool = False):
        """The GPU part of one case: staged file bytes -> (labels, probabilities or None, properties)."""
        data, props = rw.decode(staged)
        seg_prev = rw.decode(staged_prev)[0] if staged_prev is not None else None
        if staged.fnames and self.verbose:
            print(f'predicting {os.path.basename(staged.fnames[0])}')
        return self._predict_case(data, props, seg_prev, save_probabilities, for_file=for_file)

    @staticmethod
    def _result(seg, probs, save_probabilities):
        return (seg, probs) if save_probabilities else seg

    def predict_from_files(self,
                           list_of_lists_or_source_folder: Union[str, List[List[str]]],
                           output_folder_or_list_of_truncated_output_files: Union[str, None, List[str]],
                           save_probabilities: bool = False,
                           overwrite: bool = True,
                           num_processes_preprocessing: int = 3,
                           num_processes_segmentation_export: int = 3,
                           folder_with_segs_from_prev_stage: str = None,
                           num_parts: int = 1,
                           part_id: int = 0):
        """predict_from_raw_data.py:207-268 with every numerical step on the device.  Host work overlaps the GPU: one
        reader thread inflates case i + 1 into pinned memory and one writer thread compresses case i - 1 while the
        calling thread - the only one that touches the GPU - runs case i.  The two ``num_processes_*`` arguments only say
        whether those threads exist (0: that side runs inline); no process is started.  With an output target the files
        are written and None entries returned like the reference's export; without one the label maps are returned (or
        ``(labels, probabilities)``)."""
        assert part_id <= num_parts, ('Part ID must be smaller than num_parts. Remember that we start counting with 0. '
                                      'So if there are 3 parts then valid part IDs are 0, 1, 2')
        kwargs = dict(list_of_lists_or_source_folder=list_of_lists_or_source_folder,
                      output_folder_or_list_of_truncated_output_files=output_folder_or_list_of_truncated_output_files,
                      save_probabilities=save_probabilities, overwrite=overwrite,
                      num_processes_preprocessing=num_processes_preprocessing,
                      num_processes_segmentation_export=num_processes_segmentation_export,
                      folder_with_segs_from_prev_stage=folder_with_segs_from_prev_stage, num_parts=num_parts, part_id=part_id)
        cases, truncated, prev = self._prepare_files_run(kwargs, sequential=False)
        if len(cases) == 0:
            return
        return self._predict_cases(cases, truncated, prev, save_probabilities,
                                   read_thread=int(num_processes_preprocessing) > 0,
                                   write_thread=int(num_processes_segmentation_export) > 0)

    def predict_from_files_sequential(self,
                                      list_of_lists_or_source_folder: Union[str, List[List[str]]],
                                      output_folder_or_list_of_truncated_output_files: Union[str, None, List[str]],
                                      save_probabilities: bool = False,
                                      overwrite: bool = True,
                                      folder_with_segs_from_prev_stage: str = None):
        """predict_from_raw_data.py:682-767: the same work as ``predict_from_files``, case after case on the calling thread."""
        kwargs = dict(list_of_lists_or_source_folder=list_of_lists_or_source_folder,
                      output_folder_or_list_of_truncated_output_files=output_folder_or_list_of_truncated_output_files,
                      save_probabilities=save_probabilities, overwrite=overwrite,
                      folder_with_segs_from_prev_stage=folder_with_segs_from_prev_stage)
        cases, truncated, prev = self._prepare_files_run(kwargs, sequential=True)
        if len(cases) == 0:
            return
        return self._predict_cases(cases, truncated, prev, save_probabilities, read_thread=False, write_thread=False)

    @torch.inference_mode()
    def _predict_cases(self, cases, truncated, prev, save_probabilities, read_thread: bool, write_thread: bool):
        rw = self._reader_writer()                              # (made by the calling thread)
        if truncated is None:
            truncated = [None] * len(cases)

        def stage(i):
            """Headers and pinned buffers on this thread; the bytes on the reader thread (or here)."""
            staged = rw.stage(cases[i], slot=2 * (i % 2))
            staged_prev = rw.stage([prev[i]], slot=2 * (i % 2) + 1) if prev[i] is not None else None
            return lambda: (staged.fill(), staged_prev.fill() if staged_prev is not None else None)

        def run(i, filled):
            seg, probs, props = self._run_staged_case(rw, *filled, save_probabilities, for_file=truncated[i] is not None)
            if truncated[i] is None:
                return self._result(seg, probs, save_probabilities), None
            return None, (lambda: self._export_case(seg, probs, props, truncated[i]))

        return run_pipeline(len(cases), stage, run, read_thread, write_thread)


def get_identifiers_from_splitted_dataset_folder(folder: str, file_ending: str):
    """utilities/utils.py:27-34: the sorted unique case identifiers of a folder of ``<case>_XXXX<ending>`` files."""
    files = sorted(i for i in os.listdir(folder) if os.path.isfile(os.path.join(folder, i)) and i.endswith(file_ending))
    crop = len(file_ending) + 5
    return sorted(set(i[:-crop] for i in files))


def create_lists_from_splitted_dataset_folder(folder: str, file_ending: str, identifiers: List[str] = None,
                                              num_processes: int = 12) -> List[List[str]]:
    """utilities/utils.py:42-56: per case the sorted files ``<case>_dddd<ending>`` (four digits).  ``num_processes`` is
    accepted and ignored: no process is started."""
    import re
    if identifiers is None:
        identifiers = get_identifiers_from_splitted_dataset_folder(folder, file_ending)
    files = sorted(i for i in os.listdir(folder) if os.path.isfile(os.path.join(folder, i)) and i.endswith(file_ending))
    out = []
    for ident in identifiers:
        p = re.compile(re.escape(ident) + r'_\d\d\d\d' + re.escape(file_ending))
        out.append([os.path.join(folder, i) for i in files if p.fullmatch(i)])
    return out
