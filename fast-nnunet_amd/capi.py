"""ctypes binding of the C ABI in ``include/fnn.h`` (``csrc/libfnn_hip.so``).

This is the stub a maintainer of the reference would add to call the engine
from ``nnUNetPredictor``.  There is no CPU fallback: if the
HIP library is missing or no GPU is visible the calls raise.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import List, Optional, Sequence, Tuple

import numpy as np

FNN_MAX_STAGES = 8
FNN_OK, FNN_E_INVALID, FNN_E_HIP, FNN_E_INF, FNN_E_UNSUPPORTED, FNN_E_STATE = 0, -1, -2, -3, -4, -5
FNN_NET_PLAIN, FNN_NET_RESENC = 0, 1
FNN_PREC_F16, FNN_PREC_F8 = 0, 1
FNN_ACC_FP16_REFERENCE, FNN_ACC_FP32, FNN_ACC_FP16_AUTOCAST = 0, 1, 2
FNN_OUT_F16, FNN_OUT_F32 = 0, 1
FNN_LABELS_ARGMAX, FNN_LABELS_REGIONS = 0, 1
FNN_LABEL_U8, FNN_LABEL_U16 = 0, 1
FNN_INTERP_LINEAR, FNN_INTERP_NEAREST_EXACT, FNN_INTERP_OTHER = 0, 1, 2
FNN_RESAMPLE_DEFAULT, FNN_RESAMPLE_TORCH = 0, 1
FNN_NORM_NONE, FNN_NORM_ZSCORE, FNN_NORM_CT, FNN_NORM_RESCALE01, FNN_NORM_RGB01 = 0, 1, 2, 3, 4

_HERE = os.path.dirname(os.path.abspath(__file__))
# FNN_LIB: another build of the same library (A-B comparisons of two builds inside one GPU session) - like every FNN_* switch
# of the library itself (csrc/knob.hip, fnn_knob) honoured only next to FNN_KNOBS=1: an embedding process's environment
# does not choose the code that runs
_KNOBS = os.environ.get('FNN_KNOBS', '0') not in ('', '0')
LIB_PATH = (os.environ.get('FNN_LIB') if _KNOBS else None) or os.path.join(_HERE, 'csrc', 'libfnn_hip.so')


class ArchDesc(C.Structure):
    _fields_ = [('kind', C.c_int32), ('n_stages', C.c_int32), ('in_channels', C.c_int32), ('num_heads', C.c_int32),
                ('features', C.c_int32 * FNN_MAX_STAGES),
                ('kernels', (C.c_int32 * 3) * FNN_MAX_STAGES),
                ('strides', (C.c_int32 * 3) * FNN_MAX_STAGES),
                ('n_conv_enc', C.c_int32 * FNN_MAX_STAGES),
                ('n_conv_dec', C.c_int32 * FNN_MAX_STAGES),
                ('patch', C.c_int32 * 3),
                ('eps', C.c_float), ('slope', C.c_float), ('spatial_dims', C.c_int32), ('precision', C.c_int32)]


class NormDesc(C.Structure):
    _fields_ = [('scheme', C.c_int32), ('mean', C.c_float), ('std', C.c_float), ('lower', C.c_float), ('upper', C.c_float),
                ('use_mask', C.c_int32)]


class ResampleDesc(C.Structure):
    _fields_ = [('order', C.c_int32), ('separate_axis', C.c_int32), ('order_z', C.c_int32), ('dtype', C.c_int32)]


class ResampleTorchDesc(C.Structure):
    _fields_ = [('dtype', C.c_int32), ('separate_axis', C.c_int32), ('memefficient', C.c_int32), ('mode', C.c_int32),
                ('aniso_axis_mode', C.c_int32)]


class EnsembleMember(C.Structure):
    """fnn_ensemble_member: one member's logits on its own network grid (transposed axes)."""
    _fields_ = [('logits', C.c_void_p), ('shape', C.c_int64 * 3), ('dtype', C.c_int32), ('family', C.c_int32),
                ('separate_axis', C.c_int32)]


class Opts(C.Structure):
    _fields_ = [('tile_step_size', C.c_double), ('use_gaussian', C.c_int32), ('n_mirror_axes', C.c_int32),
                ('mirror_axes', C.c_int32 * 3), ('accum', C.c_int32), ('out_dtype', C.c_int32),
                ('batch', C.c_int32), ('stream', C.c_void_p)]


class Profile(C.Structure):
    _fields_ = [('total_ms', C.c_double), ('conv_ms', C.c_double), ('stem_ms', C.c_double),
                ('tconv_ms', C.c_double), ('head_ms', C.c_double), ('finalize_ms', C.c_double),
                ('conv_launches', C.c_int64), ('conv_flops', C.c_double), ('n_patches', C.c_int64),
                ('conv_bytes', C.c_double)]


EXPORTS = ['fnn_abi_version', 'fnn_last_error', 'fnn_create', 'fnn_destroy', 'fnn_weight_count', 'fnn_load_weights',
           'fnn_set_gaussian', 'fnn_predict_volume', 'fnn_predict_volume_ensemble', 'fnn_predict_labels',
           'fnn_set_label_rule', 'fnn_accumulator_channels', 'fnn_accumulate_patches', 'fnn_normalize_box', 'fnn_labels_box', 'fnn_feature_channels', 'fnn_patch_features', 'fnn_gather_box', 'fnn_pack_regions', 'fnn_unpack_regions', 'fnn_forward_patches', 'fnn_argmax_labels', 'fnn_nonzero_bbox', 'fnn_preprocess', 'fnn_revert_labels', 'fnn_export_probabilities', 'fnn_resample', 'fnn_resample_torch', 'fnn_resample_torch_seg', 'fnn_resample_labels', 'fnn_keep_largest_components', 'fnn_remove_small_components', 'fnn_fill_holes', 'fnn_binary_morphology', 'fnn_ensemble_export', 'fnn_average_probabilities', 'fnn_ensemble_resample_export', 'fnn_confusion_counts', 'fnn_surface_count', 'fnn_surface_distances', 'fnn_instance_overlaps', 'fnn_mesh_count', 'fnn_mesh_emit', 'fnn_mesh_decimate', 'fnn_decode_voxels', 'fnn_decode_labels', 'fnn_reorient', 'fnn_deflate_bound', 'fnn_deflate_labels', 'fnn_deflate_labels_dyn', 'fnn_deflate_masks_work_bytes', 'fnn_deflate_masks_count', 'fnn_deflate_masks_emit', 'fnn_inflate_segments', 'fnn_inflate_segments_dyn', 'fnn_inflate_find_blocks', 'fnn_inflate_stream', 'fnn_compute_steps', 'fnn_plan_volume', 'fnn_fp8_e4m3_encode',
           'fnn_set_profiling', 'fnn_get_profile', 'fnn_kernel_log', 'fnn_profile_launches', 'fnn_layer_table', 'fnn_plan_table', 'fnn_patch_work', 'fnn_op_conv3d', 'fnn_op_conv_transpose3d', 'fnn_op_avgpool', 'fnn_op_combine', 'fnn_op_seg_head', 'fnn_op_patch_acc', 'fnn_op_patch_input', 'fnn_op_stem', 'fnn_op_conv_fused', 'fnn_op_quotient_check', 'fnn_op_last_kernels', 'fnn_clock_probe_start', 'fnn_clock_probe_stop']

_lib = None


class EngineError(RuntimeError):
    pass


def load_library() -> C.CDLL:
    """Load ``libfnn_hip.so``; raises if it was not built (no silent fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.isfile(LIB_PATH):
        raise EngineError(f'{LIB_PATH} is missing: build it with `make -C {os.path.dirname(LIB_PATH)}` '
                          f'(or `python -c "import __graft_entry__ as g; g.build()"`). '
                          f'There is no CPU fallback for the inference engine.')
    lib = C.CDLL(LIB_PATH)
    vp, i32, i64, f32p = C.c_void_p, C.c_int, C.c_int64, C.POINTER(C.c_float)
    lib.fnn_abi_version.restype = i32
    lib.fnn_last_error.restype = C.c_char_p
    lib.fnn_last_error.argtypes = [vp]
    lib.fnn_create.argtypes = [C.POINTER(ArchDesc), i32, i32, C.POINTER(vp)]
    lib.fnn_destroy.argtypes = [vp]
    lib.fnn_destroy.restype = None
    lib.fnn_weight_count.argtypes = [vp]
    lib.fnn_weight_count.restype = i64
    lib.fnn_load_weights.argtypes = [vp, i32, vp, i64]
    lib.fnn_set_gaussian.argtypes = [vp, vp, i64]
    lib.fnn_predict_volume.argtypes = [vp, i32, vp, C.POINTER(i64), C.POINTER(Opts), vp]
    lib.fnn_predict_volume_ensemble.argtypes = [vp, i32, vp, C.POINTER(i64), C.POINTER(Opts), vp]
    lib.fnn_predict_labels.argtypes = [vp, i32, vp, C.POINTER(i64), C.POINTER(Opts), vp]
    lib.fnn_set_label_rule.argtypes = [vp, i32, C.POINTER(i32), i32, i32]
    lib.fnn_accumulator_channels.argtypes = [vp]
    lib.fnn_accumulator_channels.restype = i64
    P64 = C.POINTER(i64)
    lib.fnn_accumulate_patches.argtypes = [vp, i32, vp, P64, C.POINTER(Opts), P64, i64, P64, P64, vp]
    lib.fnn_normalize_box.argtypes = [vp, vp, P64, C.POINTER(Opts), P64, P64, P64, P64, vp]
    lib.fnn_labels_box.argtypes = [vp, vp, P64, C.POINTER(Opts), P64, P64, P64, P64, vp]
    lib.fnn_feature_channels.argtypes = [vp]
    lib.fnn_feature_channels.restype = i64
    lib.fnn_patch_features.argtypes = [vp, i32, vp, P64, C.POINTER(Opts), P64, i64, vp, vp, i64, i64]
    lib.fnn_gather_box.argtypes = [vp, i32, vp, vp, C.POINTER(C.c_int32), i64, P64, C.POINTER(Opts), P64, P64, vp, vp]
    lib.fnn_pack_regions.argtypes = [vp, vp, i64, vp, i64, vp, vp]
    lib.fnn_unpack_regions.argtypes = [vp, vp, i64, vp, i64, vp, vp]
    lib.fnn_forward_patches.argtypes = [vp, i32, vp, i32, vp, vp]
    lib.fnn_argmax_labels.argtypes = [vp, vp, i32, i32, i64, vp, vp]
    lib.fnn_nonzero_bbox.argtypes = [vp, C.POINTER(i64), C.POINTER(i32), C.POINTER(i64), vp]
    lib.fnn_preprocess.argtypes = [vp, C.POINTER(i64), C.POINTER(i32), C.POINTER(i64), C.POINTER(NormDesc), vp, vp]
    lib.fnn_revert_labels.argtypes = [vp, i32, C.POINTER(i64), C.POINTER(i64), C.POINTER(i32), vp, vp]
    lib.fnn_export_probabilities.argtypes = [vp, i32, i32, C.POINTER(C.c_int32), C.POINTER(i64), C.POINTER(i64),
                                             C.POINTER(i32), vp, vp, i32, vp]
    lib.fnn_resample.argtypes = [vp, C.POINTER(i64), C.POINTER(i64), C.POINTER(ResampleDesc), vp, vp]
    lib.fnn_resample_torch.argtypes = [vp, C.POINTER(i64), C.POINTER(i64), C.POINTER(ResampleTorchDesc), vp, vp]
    lib.fnn_resample_torch_seg.argtypes = [vp, C.POINTER(i64), C.POINTER(i64), C.POINTER(ResampleTorchDesc), vp, vp]
    lib.fnn_resample_labels.argtypes = [vp, i32, C.POINTER(i64), C.POINTER(i64), i32, i32, vp, i32, vp, i32, vp]
    lib.fnn_keep_largest_components.argtypes = [vp, i32, C.POINTER(i64), C.POINTER(C.c_int32), i32, i32, i32, C.POINTER(i64), vp]
    if hasattr(lib, 'fnn_remove_small_components'):                # (absent from an older build picked with FNN_LIB for an A-B)
        lib.fnn_remove_small_components.argtypes = [vp, i32, C.POINTER(i64), C.POINTER(C.c_int32), i32, i32, i32, C.POINTER(i64), i32,
                                                    C.POINTER(i64), vp]
        lib.fnn_fill_holes.argtypes = [vp, i32, C.POINTER(i64), C.POINTER(C.c_int32), i32, i32, i32, i32, C.POINTER(i64), vp]
    if hasattr(lib, 'fnn_binary_morphology'):
        lib.fnn_binary_morphology.argtypes = [vp, i32, C.POINTER(i64), C.POINTER(C.c_int32), i32, i32, i32, i32, i32, i32, i32, i32,
                                              C.POINTER(i64), vp]
    lib.fnn_ensemble_export.argtypes = [C.POINTER(vp), C.POINTER(C.c_int32), i32, i32, C.POINTER(C.c_int32), C.POINTER(i64),
                                        C.POINTER(i64), C.POINTER(C.c_int32), vp, vp, i32, vp]
    lib.fnn_average_probabilities.argtypes = [C.POINTER(vp), i32, i32, C.POINTER(C.c_int32), i64, vp, vp, i32, vp]
    lib.fnn_ensemble_resample_export.argtypes = [C.POINTER(EnsembleMember), i32, i32, C.POINTER(C.c_int32), C.POINTER(i64),
                                                 C.POINTER(i64), C.POINTER(C.c_int32), vp, vp, i32, vp]
    lib.fnn_confusion_counts.argtypes = [vp, C.POINTER(vp), i32, i32, i64, C.POINTER(C.c_int32), i32, i32, i32,
                                         C.POINTER(i64), vp]
    lib.fnn_surface_count.argtypes = [vp, vp, i32, C.POINTER(i64), C.POINTER(C.c_uint8), i32, i32, C.POINTER(i64), C.POINTER(i64), vp]
    lib.fnn_surface_distances.argtypes = [vp, vp, i32, C.POINTER(i64), C.POINTER(C.c_uint8), i32, i32, C.POINTER(C.c_double), vp, i64, vp]
    if hasattr(lib, 'fnn_instance_overlaps'):                      # (absent from an older build picked with FNN_LIB for an A-B)
        lib.fnn_instance_overlaps.argtypes = [vp, vp, i32, C.POINTER(i64), C.POINTER(C.c_int32), i32, i32, vp, i64, C.POINTER(i64), vp]
    if hasattr(lib, 'fnn_mesh_count'):                             # (absent from an older build picked with FNN_LIB for an A-B)
        lib.fnn_mesh_count.argtypes = [vp, i32, C.POINTER(i64), C.POINTER(C.c_uint8), i32, i32, C.POINTER(i64), C.POINTER(i64), vp]
        lib.fnn_mesh_emit.argtypes = [vp, i32, C.POINTER(i64), C.POINTER(C.c_uint8), i32, i32, C.POINTER(C.c_double), i32, i32, vp, i64,
                                      vp, i64, vp, vp]
    if hasattr(lib, 'fnn_mesh_decimate'):
        lib.fnn_mesh_decimate.argtypes = [vp, i64, vp, vp, i64, C.POINTER(i64), i32, C.c_double, i32, vp, i64, vp, i64, vp, C.POINTER(i64),
                                          C.POINTER(i64), vp]
    lib.fnn_decode_voxels.argtypes =[vp, i32, i32, i64, i32, C.c_double, C.c_double, vp, vp]
    lib.fnn_decode_labels.argtypes = [vp, i32, i32, i64, i32, C.c_double, C.c_double, i32, vp, vp, vp]
    lib.fnn_reorient.argtypes = [vp, i32, C.POINTER(i64), C.POINTER(C.c_int32), C.POINTER(C.c_int32), vp, vp]
    lib.fnn_deflate_bound.argtypes = [i64]
    lib.fnn_deflate_bound.restype = i64
    lib.fnn_deflate_labels.argtypes = [vp, i32, i64, i32, vp, i64, C.POINTER(i64), C.POINTER(i32), C.POINTER(C.c_uint32), vp]
    lib.fnn_deflate_labels_dyn.argtypes = [vp, i32, i64, i32, vp, i64, C.POINTER(i64), C.POINTER(i32), C.POINTER(C.c_uint32), C.POINTER(i64), vp]
    lib.fnn_deflate_masks_work_bytes.argtypes = [i64, i32]
    lib.fnn_deflate_masks_work_bytes.restype = i64
    lib.fnn_deflate_masks_count.argtypes = [vp, i32, i64, C.POINTER(C.c_int32), i32, vp, i64, C.POINTER(i64), C.POINTER(C.c_uint32), vp]
    lib.fnn_deflate_masks_emit.argtypes = [vp, i32, i64, C.POINTER(C.c_int32), i32, vp, vp, i64, vp]
    lib.fnn_inflate_segments.argtypes = [vp, i64, C.POINTER(i64), i64, vp, i64, C.POINTER(C.c_uint32), C.POINTER(C.c_int32), vp]
    lib.fnn_inflate_segments_dyn.argtypes = lib.fnn_inflate_segments.argtypes
    lib.fnn_inflate_find_blocks.argtypes = [vp, i64, vp, i64, C.POINTER(i64), vp]
    lib.fnn_inflate_stream.argtypes = [vp, i64, vp, i64, C.POINTER(C.c_uint32), C.POINTER(C.c_int32), vp]
    lib.fnn_compute_steps.argtypes = [i64, i64, C.c_double, C.POINTER(i64), i32]
    lib.fnn_plan_volume.argtypes = [C.POINTER(C.c_int32), C.POINTER(i64), C.c_double, C.POINTER(i64), C.POINTER(i64),
                                    C.POINTER(i64), C.POINTER(C.c_int32), i64]
    lib.fnn_fp8_e4m3_encode.argtypes = [vp, i64, vp]
    lib.fnn_set_profiling.argtypes = [vp, i32]
    lib.fnn_get_profile.argtypes = [vp, C.POINTER(Profile)]
    lib.fnn_kernel_log.argtypes = [vp, C.c_char_p, i64]
    lib.fnn_kernel_log.restype = i64
    for name in ('fnn_profile_launches', 'fnn_layer_table'):       # (absent from an older build picked with FNN_LIB for an A-B)
        if hasattr(lib, name):
            fn = getattr(lib, name)
            fn.argtypes = [vp, C.c_char_p, i64]
            fn.restype = i64
    lib.fnn_plan_table.argtypes = [C.POINTER(ArchDesc), i32, C.c_char_p, i64]
    lib.fnn_plan_table.restype = i64
    lib.fnn_patch_work.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    I3 = C.POINTER(C.c_int)
    lib.fnn_op_conv3d.argtypes = [i32, i32, I3, f32p, i32, f32p, f32p, C.c_float, f32p, i32, f32p, f32p, C.c_float,
                                  f32p, f32p, i32, I3, I3, f32p, C.POINTER(C.c_double)]
    lib.fnn_op_conv_transpose3d.argtypes = [i32, i32, I3, f32p, i32, f32p, f32p, C.c_float, f32p, f32p, i32, I3, f32p]
    L3, u16p = C.POINTER(C.c_longlong), C.POINTER(C.c_uint16)
    if hasattr(lib, 'fnn_op_avgpool'):                             # (absent from an older build picked with FNN_LIB for an A-B)
        lib.fnn_op_avgpool.argtypes = [i32, i32, I3, f32p, i32, f32p, f32p, C.c_float, I3, i32, i32, f32p]
        lib.fnn_op_combine.argtypes = [i32, i32, I3, i32, f32p, f32p, f32p, C.c_float, f32p, f32p, f32p, C.c_float, C.c_float, I3,
                                       i32, i32, i32, i32, f32p, f32p]
        lib.fnn_op_seg_head.argtypes = [i32, i32, i32, I3, f32p, f32p, f32p, C.c_float, i32, f32p, f32p, i32, i32, I3, u16p,
                                        vp, i32, L3, I3, I3, f32p, C.POINTER(C.c_int)]
        lib.fnn_op_patch_acc.argtypes = [i32, f32p, i32, I3, i32, u16p, vp, i32, L3, I3]
        lib.fnn_op_patch_input.argtypes = [i32, f32p, i32, i32, L3, i32, I3, I3, I3, i32, i32, u16p]
    if hasattr(lib, 'fnn_op_stem'):                                # (absent from an older build picked with FNN_LIB for an A-B)
        f64p = C.POINTER(C.c_double)
        lib.fnn_op_stem.argtypes = [i32, f32p, i32, i32, L3, i32, I3, I3, I3, f32p, f32p, i32, I3, f32p, f64p]
        lib.fnn_op_conv_fused.argtypes = [i32, i32, i32, I3, f32p, i32, L3, I3, I3, f32p, i32, I3, f32p, f32p, f32p, C.c_float,
                                          f32p, f32p, f32p, f32p, C.c_float, f32p, f32p, I3, f32p, f64p]
    lib.fnn_op_quotient_check.argtypes = [i32, C.POINTER(C.c_uint64)]
    lib.fnn_op_last_kernels.argtypes = [C.c_char_p, i32]
    lib.fnn_clock_probe_start.argtypes = [i32, C.c_double, C.POINTER(C.c_void_p)]
    lib.fnn_clock_probe_stop.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    if lib.fnn_abi_version() != 4:
        raise EngineError('libfnn_hip.so has an unexpected ABI version')
    _lib = lib
    return lib


def _err(lib, handle) -> str:
    msg = lib.fnn_last_error(handle)
    return msg.decode() if msg else ''


def check(rc: int, lib, handle=None):
    """Map C status codes onto the exception types the reference raises."""
    if rc >= 0:
        return rc
    msg = _err(lib, handle)
    if rc == FNN_E_INVALID:
        raise AssertionError(msg)
    if rc == FNN_E_UNSUPPORTED:
        raise NotImplementedError(msg)
    raise RuntimeError(msg)            # FNN_E_INF, FNN_E_HIP, FNN_E_STATE


_LAYER_KEYS = ('index', 'type', 'cin', 'cout', 'kernel', 'stride', 'in_dims', 'out_dims', 'flops', 'bytes', 'fused', 'picked')
_LAYER_CONV = (int, str, int, int, str, str, str, str, float, float, int, str)


def _layer_rows(rows):
    return [dict((k, c(v)) for k, c, v in zip(_LAYER_KEYS, _LAYER_CONV, r)) for r in rows]


def plan_table(desc: ArchDesc, max_batch: int):
    """The layer plan fnn_create(desc, device, max_batch) would make, without a GPU: rows as Engine.layer_table()."""
    lib = load_library()
    n = check(lib.fnn_plan_table(C.byref(desc), int(max_batch), None, 0), lib)
    buf = C.create_string_buffer(int(n))
    lib.fnn_plan_table(C.byref(desc), int(max_batch), buf, n)
    return _layer_rows(r.split('\t') for r in buf.value.decode().split('\n') if r)


def _f32p(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_float))


def fp8_e4m3_encode(x: np.ndarray) -> np.ndarray:
    """float32 -> OCP e4m3 bytes with the library's host quantiser (FNN_PREC_F8 weight packing)."""
    lib = load_library()
    x = np.ascontiguousarray(x, np.float32)
    out = np.empty(x.shape, np.uint8)
    check(lib.fnn_fp8_e4m3_encode(x.ctypes.data, x.size, out.ctypes.data), lib)
    return out


def compute_steps(image_size: int, patch_size: int, step: float):
    lib = load_library()
    buf = (C.c_int64 * 4096)()
    n = check(lib.fnn_compute_steps(int(image_size), int(patch_size), float(step), buf, 4096), lib)
    return [int(buf[i]) for i in range(n)]


def plan_volume(patch: Sequence[int], shape_sp: Sequence[int], step: float):
    """-> (padded shape, low pads, origins [n,3]) exactly as the engine will visit them.  A patch with two
    entries is a `2d` configuration: every slice of the first axis, tiles over the other two."""
    lib = load_library()
    patch = [0, *patch] if len(patch) == 2 else list(patch)
    p = (C.c_int32 * 3)(*[int(i) for i in patch])
    s = (C.c_int64 * 3)(*[int(i) for i in shape_sp])
    padded, lo, n = (C.c_int64 * 3)(), (C.c_int64 * 3)(), C.c_int64(0)
    check(lib.fnn_plan_volume(p, s, float(step), padded, lo, C.byref(n), None, 0), lib)
    org = np.zeros((n.value, 3), dtype=np.int32)
    check(lib.fnn_plan_volume(p, s, float(step), padded, lo, C.byref(n),
                              org.ctypes.data_as(C.POINTER(C.c_int32)), n.value), lib)
    return list(padded), list(lo), org


def nonzero_bbox(raw_ptr: int, shape, transpose_forward, stream: int = 0):
    """-> [[lo, hi], ...] per TRANSPOSED axis (properties['bbox_used_for_cropping'])."""
    lib = load_library()
    bbox = (C.c_int64 * 6)()
    check(lib.fnn_nonzero_bbox(raw_ptr, (C.c_int64 * 4)(*[int(i) for i in shape]),
                               (C.c_int32 * 3)(*[int(i) for i in transpose_forward]), bbox, stream), lib)
    return [[int(bbox[2 * a]), int(bbox[2 * a + 1])] for a in range(3)]


def preprocess(raw_ptr: int, shape, transpose_forward, bbox, norms, out_ptr: int, stream: int = 0):
    """norms: one (scheme, mean, std, lower, upper[, use_mask]) per channel."""
    lib = load_library()
    nd = (NormDesc * len(norms))(*[NormDesc(int(n[0]), float(n[1]), float(n[2]), float(n[3]), float(n[4]),
                                            int(n[5]) if len(n) > 5 else 0) for n in norms])
    flat = (C.c_int64 * 6)(*[int(v) for ab in bbox for v in ab])
    check(lib.fnn_preprocess(raw_ptr, (C.c_int64 * 4)(*[int(i) for i in shape]),
                             (C.c_int32 * 3)(*[int(i) for i in transpose_forward]), flat, nd, out_ptr, stream), lib)


def revert_labels(seg_ptr: int, uint16: bool, bbox, shape_before_cropping, transpose_backward, out_ptr: int, stream: int = 0):
    lib = load_library()
    flat = (C.c_int64 * 6)(*[int(v) for ab in bbox for v in ab])
    check(lib.fnn_revert_labels(seg_ptr, FNN_LABEL_U16 if uint16 else FNN_LABEL_U8, flat,
                                (C.c_int64 * 3)(*[int(i) for i in shape_before_cropping]),
                                (C.c_int32 * 3)(*[int(i) for i in transpose_backward]), out_ptr, stream), lib)


def export_probabilities(logits_ptr: int, half: bool, heads: int, regions_class_order, bbox, shape_before_cropping,
                         transpose_backward, probs_ptr: int, labels_ptr: int, uint16: bool, stream: int = 0):
    """Probabilities + labels on the original grid from logits of the cropped grid (export_prediction.py:36-70)."""
    lib = load_library()
    order = None
    if regions_class_order is not None:
        assert len(regions_class_order) == heads
        order = (C.c_int32 * heads)(*[int(c) for c in regions_class_order])
    flat = (C.c_int64 * 6)(*[int(v) for ab in bbox for v in ab])
    check(lib.fnn_export_probabilities(logits_ptr, FNN_OUT_F16 if half else FNN_OUT_F32, int(heads), order, flat,
                                       (C.c_int64 * 3)(*[int(i) for i in shape_before_cropping]),
                                       (C.c_int32 * 3)(*[int(i) for i in transpose_backward]), probs_ptr, labels_ptr,
                                       FNN_LABEL_U16 if uint16 else FNN_LABEL_U8, stream), lib)


def resample(in_ptr: int, shape, new_shape, order: int, separate_axis, half: bool, out_ptr: int, stream: int = 0, order_z: int = 0):
    """resample_data_or_seg(is_seg=False) of a [C, ...] tensor (fp32, or fp16 when `half`)."""
    lib = load_library()
    d = ResampleDesc(int(order), -1 if separate_axis is None else int(separate_axis), int(order_z),
                     FNN_OUT_F16 if half else FNN_OUT_F32)
    check(lib.fnn_resample(in_ptr, (C.c_int64 * 4)(*[int(i) for i in shape]), (C.c_int64 * 3)(*[int(i) for i in new_shape]),
                           C.byref(d), out_ptr, stream), lib)


def _interp_mode(name: str) -> int:
    return {'linear': FNN_INTERP_LINEAR, 'nearest-exact': FNN_INTERP_NEAREST_EXACT}.get(name, FNN_INTERP_OTHER)


def resample_torch(in_ptr: int, shape, new_shape, separate_axis, half: bool, out_ptr: int, stream: int = 0, is_seg: bool = False,
                   memefficient: bool = False, mode: str = 'linear', aniso_axis_mode: str = 'nearest-exact'):
    """resample_torch_fornnunet of a [C, ...] tensor: fp32 / fp16 (`half`) images and logits, or with `is_seg` int16 label
    maps (the fp16-argmax rule, or the `memefficient` one).  Asynchronous on `stream`."""
    lib = load_library()
    d = ResampleTorchDesc(FNN_OUT_F16 if half else FNN_OUT_F32, -1 if separate_axis is None else int(separate_axis),
                          int(bool(memefficient)), _interp_mode(mode), _interp_mode(aniso_axis_mode))
    fn = lib.fnn_resample_torch_seg if is_seg else lib.fnn_resample_torch
    check(fn(in_ptr, (C.c_int64 * 4)(*[int(i) for i in shape]), (C.c_int64 * 3)(*[int(i) for i in new_shape]),
             C.byref(d), out_ptr, stream), lib)


def resample_labels(logits_ptr: int, half: bool, shape, new_shape, family: int, separate_axis, order_ptr: Optional[int],
                    n_regions: int, labels_ptr: int, uint16: bool, stream: int = 0):
    """fnn_resample_labels: logits [heads, *shape[1:]] of the network grid (fp32, or fp16 when `half`) -> labels [new_shape],
    resampled by `family` (FNN_RESAMPLE_DEFAULT: order 1, order_z 0; FNN_RESAMPLE_TORCH) and put through the label rule in
    one pass.  order_ptr: None (argmax) or n_regions = heads int32 of regions_class_order in DEVICE memory.  Asynchronous on
    `stream`; op_last_kernels() names the kernel that ran."""
    lib = load_library()
    check(lib.fnn_resample_labels(logits_ptr, FNN_OUT_F16 if half else FNN_OUT_F32, (C.c_int64 * 4)(*[int(i) for i in shape]),
                                  (C.c_int64 * 3)(*[int(i) for i in new_shape]), int(family),
                                  -1 if separate_axis is None else int(separate_axis), order_ptr, int(n_regions), labels_ptr,
                                  FNN_LABEL_U16 if uint16 else FNN_LABEL_U8, stream), lib)


def decode_voxels(raw_ptr: int, nifti_datatype: int, byteswap: bool, n_vox: int, scale: bool, slope: float, inter: float,
                  out_ptr: int, stream: int = 0):
    """fnn_decode_voxels: n_vox voxels of a NIfTI datatype at raw_ptr (device, 16-byte aligned) -> float32 at out_ptr
    (device), asynchronous on `stream`."""
    lib = load_library()
    check(lib.fnn_decode_voxels(raw_ptr, int(nifti_datatype), int(bool(byteswap)), int(n_vox), int(bool(scale)),
                                float(slope), float(inter), out_ptr, stream), lib)


LABEL_FLAG_NOT_INTEGRAL, LABEL_FLAG_NEGATIVE, LABEL_FLAG_TOO_LARGE = 1, 2, 4


def decode_labels(raw_ptr: int, nifti_datatype: int, byteswap: bool, n_vox: int, scale: bool, slope: float, inter: float,
                  out_bytes: int, out_ptr: int, status_ptr: int, stream: int = 0):
    """fnn_decode_labels: n_vox voxels of a NIfTI datatype at raw_ptr (device, 16-byte aligned) -> uint8 (out_bytes 1) or
    uint16 (2) labels at out_ptr (device, element aligned); what is no label stores 0.  status_ptr: two int32 on the
    device - the LABEL_FLAG_* of all voxels OR-ed, the largest valid label - zeroed and written on `stream`,
    asynchronously."""
    lib = load_library()
    check(lib.fnn_decode_labels(raw_ptr, int(nifti_datatype), int(bool(byteswap)), int(n_vox), int(bool(scale)),
                                float(slope), float(inter), int(out_bytes), out_ptr, status_ptr, stream), lib)


def reorient(in_ptr: int, elem_bytes: int, shape_in, src_axis, flip, out_ptr: int, stream: int = 0):
    """fnn_reorient: the C-order 3-D array of `elem_bytes`-byte elements at in_ptr (device) flipped and permuted into
    out_ptr (device, shape ``[shape_in[a] for a in src_axis]``): ``out[i] = in[j]`` with ``j[src_axis[d]] = shape_in[src_axis[d]]
    - 1 - i[d]`` where ``flip[d]``, else ``i[d]``.  Asynchronous on `stream`."""
    lib = load_library()
    check(lib.fnn_reorient(in_ptr, int(elem_bytes), (C.c_int64 * 3)(*[int(i) for i in shape_in]),
                           (C.c_int32 * 3)(*[int(i) for i in src_axis]), (C.c_int32 * 3)(*[int(bool(i)) for i in flip]),
                           out_ptr, stream), lib)


def deflate_bound(n_bytes: int) -> int:
    """fnn_deflate_bound: an output capacity that always suffices for n_bytes of labels (host only)."""
    return int(load_library().fnn_deflate_bound(int(n_bytes)))


def deflate_labels(in_ptr: int, in_elem_bytes: int, n_elems: int, narrow_if_fits: bool, out_ptr: int, out_cap: int,
                   stream: int = 0) -> Tuple[int, int, int]:
    """fnn_deflate_labels: n_elems labels of 1 or 2 bytes at in_ptr (device, 16-byte aligned) -> a raw-deflate fragment at
    out_ptr (device, out_cap >= deflate_bound(n_elems * in_elem_bytes)).  Returns ``(bytes written, bytes per element in the
    file, CRC-32 of the file bytes)``; synchronises `stream`."""
    lib = load_library()
    out_bytes, file_elem, crc = C.c_int64(-1), C.c_int(0), C.c_uint32(0)
    check(lib.fnn_deflate_labels(in_ptr, int(in_elem_bytes), int(n_elems), int(bool(narrow_if_fits)), out_ptr, int(out_cap),
                                 C.byref(out_bytes), C.byref(file_elem), C.byref(crc), stream), lib)
    return int(out_bytes.value), int(file_elem.value), int(crc.value)


def deflate_labels_dyn(in_ptr: int, in_elem_bytes: int, n_elems: int, narrow_if_fits: bool, out_ptr: int, out_cap: int,
                       stream: int = 0) -> Tuple[int, int, int, int]:
    """fnn_deflate_labels_dyn: ``deflate_labels`` with per-chunk dynamic Huffman tables - the same arguments and refusals.
    Returns ``(bytes written, bytes per element in the file, CRC-32 of the file bytes, chunks that took their own
    tables)``; synchronises `stream`."""
    lib = load_library()
    out_bytes, file_elem, crc, dynamic = C.c_int64(-1), C.c_int(0), C.c_uint32(0), C.c_int64(-1)
    check(lib.fnn_deflate_labels_dyn(in_ptr, int(in_elem_bytes), int(n_elems), int(bool(narrow_if_fits)), out_ptr, int(out_cap),
                                     C.byref(out_bytes), C.byref(file_elem), C.byref(crc), C.byref(dynamic), stream), lib)
    return int(out_bytes.value), int(file_elem.value), int(crc.value), int(dynamic.value)


def deflate_masks_work_bytes(n_elems: int, n_labels: int) -> int:
    """fnn_deflate_masks_work_bytes: the size of the device buffer ``deflate_masks_count`` fills for ``deflate_masks_emit``
    (host only)."""
    return int(load_library().fnn_deflate_masks_work_bytes(int(n_elems), int(n_labels)))


def _label_array(labels):
    labels = [int(i) for i in labels]
    if any(not -2 ** 31 <= i < 2 ** 31 for i in labels):
        raise AssertionError('a label lies outside [0, 65535]')
    return (C.c_int32 * max(len(labels), 1))(*labels), len(labels)


def deflate_masks_count(in_ptr: int, in_elem_bytes: int, n_elems: int, labels, work_ptr: int, work_cap: int,
                        stream: int = 0) -> Tuple[List[int], List[int]]:
    """fnn_deflate_masks_count: for the map of n_elems labels of 1 or 2 bytes at in_ptr (device, 16-byte aligned) and every
    value in ``labels``, the size of the raw-deflate fragment of the mask ``map == value`` and zlib's CRC-32 of the mask
    bytes -> ``(sizes, crcs)``.  work_ptr: a device buffer of ``deflate_masks_work_bytes`` bytes that ``deflate_masks_emit``
    then reads.  Synchronises `stream`."""
    lib = load_library()
    arr, n = _label_array(labels)
    sizes, crcs = (C.c_int64 * max(n, 1))(), (C.c_uint32 * max(n, 1))()
    check(lib.fnn_deflate_masks_count(in_ptr, int(in_elem_bytes), int(n_elems), arr, n, work_ptr, int(work_cap), sizes, crcs,
                                      stream), lib)
    return [int(sizes[i]) for i in range(n)], [int(crcs[i]) for i in range(n)]


def deflate_masks_emit(in_ptr: int, in_elem_bytes: int, n_elems: int, labels, work_ptr: int, out_ptr: int, out_cap: int,
                       stream: int = 0) -> None:
    """fnn_deflate_masks_emit: the fragments ``deflate_masks_count`` sized (same map, same labels, its work buffer), one
    behind the other at out_ptr (device, any alignment, out_cap >= their sum).  The kernel runs asynchronously on `stream`."""
    lib = load_library()
    arr, n = _label_array(labels)
    check(lib.fnn_deflate_masks_emit(in_ptr, int(in_elem_bytes), int(n_elems), arr, n, work_ptr, out_ptr, int(out_cap), stream), lib)


FNN_INFLATE_SEGMENT_MAX = 16384
INFLATE_REASONS = ('OK', 'DYNAMIC', 'BTYPE3', 'FINAL', 'SYMBOL', 'NLEN', 'DISTANCE', 'OUTPUT', 'INPUT', 'END', 'CHAIN', 'SIZE')   # FNN_INFLATE_*
(FNN_INFLATE_OK, FNN_INFLATE_DYNAMIC, FNN_INFLATE_BTYPE3, FNN_INFLATE_FINAL, FNN_INFLATE_SYMBOL, FNN_INFLATE_NLEN,
 FNN_INFLATE_DISTANCE, FNN_INFLATE_OUTPUT, FNN_INFLATE_INPUT, FNN_INFLATE_END, FNN_INFLATE_CHAIN, FNN_INFLATE_SIZE) = range(12)
FNN_INFLATE_TABLES = 12                                           # fnn_inflate_segments_dyn alone
INFLATE_DYN_REASONS = INFLATE_REASONS + ('TABLES',)


def inflate_segments(in_ptr: int, in_bytes: int, starts, out_ptr: int, out_bytes: int, stream: int = 0):
    """fnn_inflate_segments: the raw deflate stream of in_bytes bytes at in_ptr (device, 16-byte aligned), claimed to be a
    chain of byte-aligned segments, inflated into the out_bytes bytes at out_ptr (device, 16-byte aligned).  ``starts``:
    host positions where a segment may start - strictly ascending from 0, all below in_bytes, false ones allowed.  Returns
    ``(status, crc32)``: with status FNN_INFLATE_OK the bytes are there and crc32 is zlib's of them; any other status says
    why the stream is not served (``INFLATE_REASONS[status]``), and the bytes are unspecified.  Synchronises the stream."""
    lib = load_library()
    arr = np.ascontiguousarray(starts, dtype=np.int64)
    crc, status = C.c_uint32(0), C.c_int32(0)
    check(lib.fnn_inflate_segments(in_ptr, int(in_bytes), arr.ctypes.data_as(C.POINTER(C.c_int64)), int(arr.size), out_ptr,
                                   int(out_bytes), C.byref(crc), C.byref(status), stream), lib)
    return int(status.value), int(crc.value)


def inflate_segments_dyn(in_ptr: int, in_bytes: int, starts, out_ptr: int, out_bytes: int, stream: int = 0):
    """fnn_inflate_segments_dyn: ``inflate_segments`` for chains whose segments may hold dynamic-Huffman blocks too (the
    fragments of ``deflate_labels_dyn``, zlib's full-flush streams of any strategy).  The same arguments and result; the
    status is one of ``INFLATE_DYN_REASONS``: never DYNAMIC, TABLES for a table header zlib's inflate would refuse."""
    lib = load_library()
    arr = np.ascontiguousarray(starts, dtype=np.int64)
    crc, status = C.c_uint32(0), C.c_int32(0)
    check(lib.fnn_inflate_segments_dyn(in_ptr, int(in_bytes), arr.ctypes.data_as(C.POINTER(C.c_int64)), int(arr.size), out_ptr,
                                       int(out_bytes), C.byref(crc), C.byref(status), stream), lib)
    return int(status.value), int(crc.value)


def inflate_find_blocks(in_ptr: int, in_bytes: int, positions_ptr: int = 0, cap: int = 0, stream: int = 0) -> int:
    """fnn_inflate_find_blocks: the bit positions of the raw deflate stream of in_bytes bytes at in_ptr (device, 16-byte
    aligned) at which a decode may begin - bit 0 and wherever a non-final dynamic block's table header stands that zlib
    would accept.  Returns how many there are; the first ``min(n, cap)`` are written, ascending, to the ``cap`` int64 at
    positions_ptr (device).  Synchronises the stream."""
    lib = load_library()
    n = C.c_int64(0)
    check(lib.fnn_inflate_find_blocks(in_ptr, int(in_bytes), positions_ptr or None, int(cap), C.byref(n), stream), lib)
    return int(n.value)


def inflate_stream(in_ptr: int, in_bytes: int, out_ptr: int, out_bytes: int, stream: int = 0):
    """fnn_inflate_stream: any raw deflate stream of in_bytes bytes at in_ptr (device, 16-byte aligned) - what zlib writes -
    inflated into the out_bytes bytes at out_ptr (device, 16-byte aligned), speculatively from every position
    ``inflate_find_blocks`` finds.  Returns ``(status, crc32)`` as ``inflate_segments`` does; the status is one of
    ``INFLATE_DYN_REASONS``.  Synchronises the stream."""
    lib = load_library()
    crc, status = C.c_uint32(0), C.c_int32(0)
    check(lib.fnn_inflate_stream(in_ptr, int(in_bytes), out_ptr, int(out_bytes), C.byref(crc), C.byref(status), stream), lib)
    return int(status.value), int(crc.value)


def keep_largest_components(labels_ptr: int, uint16: bool, shape, group_of_label, n_groups: int, background_label: int,
                            stream: int = 0):
    """fnn_keep_largest_components on a device label map [X, Y, Z] in place; returns the voxels removed per set."""
    lib = load_library()
    table = np.ascontiguousarray(group_of_label, dtype=np.int32)
    removed = np.zeros(max(int(n_groups), 1), np.int64)
    check(lib.fnn_keep_largest_components(labels_ptr, FNN_LABEL_U16 if uint16 else FNN_LABEL_U8,
                                          (C.c_int64 * 3)(*[int(i) for i in shape]),
                                          table.ctypes.data_as(C.POINTER(C.c_int32)), int(table.size), int(n_groups),
                                          int(background_label), removed.ctypes.data_as(C.POINTER(C.c_int64)), stream), lib)
    return removed[:int(n_groups)]


def remove_small_components(labels_ptr: int, uint16: bool, shape, group_of_label, n_groups: int, background_label: int, min_size,
                            connectivity: int = 26, stream: int = 0):
    """fnn_remove_small_components on a device label map [X, Y, Z] in place: per set, components below ``min_size[set]``
    voxels become background; returns the voxels removed per set."""
    lib = load_library()
    table = np.ascontiguousarray(group_of_label, dtype=np.int32)
    sizes = np.ascontiguousarray(min_size, dtype=np.int64)
    if sizes.shape != (int(n_groups),):
        raise ValueError('min_size must have one entry per set')
    sizes = np.concatenate([sizes, np.zeros(1, np.int64)])                  # never an empty buffer
    removed = np.zeros(max(int(n_groups), 1), np.int64)
    check(lib.fnn_remove_small_components(labels_ptr, FNN_LABEL_U16 if uint16 else FNN_LABEL_U8,
                                          (C.c_int64 * 3)(*[int(i) for i in shape]),
                                          table.ctypes.data_as(C.POINTER(C.c_int32)), int(table.size), int(n_groups),
                                          int(background_label), sizes.ctypes.data_as(C.POINTER(C.c_int64)), int(connectivity),
                                          removed.ctypes.data_as(C.POINTER(C.c_int64)), stream), lib)
    return removed[:int(n_groups)]


def fill_holes(labels_ptr: int, uint16: bool, shape, in_set, background_label: int, fill_label: int, border_axes: int = 7,
               stream: int = 0) -> int:
    """fnn_fill_holes on a device label map [X, Y, Z] in place: ``in_set[v]`` is 0 where label value v belongs to the set and
    -1 where not; background voxels in the set's holes become ``fill_label``.  ``border_axes``: bit a - the faces of axis a
    are borders (7 for a 3-D map, 6 for a 2-D map carried as [1, Y, Z]).  Returns the number of voxels filled."""
    lib = load_library()
    table = np.ascontiguousarray(in_set, dtype=np.int32)
    filled = C.c_int64(0)
    check(lib.fnn_fill_holes(labels_ptr, FNN_LABEL_U16 if uint16 else FNN_LABEL_U8, (C.c_int64 * 3)(*[int(i) for i in shape]),
                             table.ctypes.data_as(C.POINTER(C.c_int32)), int(table.size), int(background_label), int(fill_label),
                             int(border_axes), C.byref(filled), stream), lib)
    return int(filled.value)


FNN_MORPH_DILATE, FNN_MORPH_ERODE, FNN_MORPH_OPEN, FNN_MORPH_CLOSE = 0, 1, 2, 3


def binary_morphology(labels_ptr: int, uint16: bool, shape, in_set, op: int, connectivity: int, iterations: int, border_value: int,
                      background_label: int, fill_label: int, axes: int = 7, stream: int = 0) -> int:
    """fnn_binary_morphology on a device label map [X, Y, Z] in place: ``in_set[v]`` is 0 where label value v belongs to the set
    and -1 where not; ``op`` is FNN_MORPH_DILATE / ERODE / OPEN / CLOSE with scipy's structure of ``connectivity`` 6 / 18 / 26,
    ``iterations`` and ``border_value``.  Dilation and closing give ``fill_label`` to the background voxels they add, erosion and
    opening ``background_label`` to the voxels they remove.  ``axes``: bit a - the structure spans axis a (7 for a 3-D map, 6
    for a 2-D map carried as [1, Y, Z]).  Returns the number of voxels written."""
    lib = load_library()
    table = np.ascontiguousarray(in_set, dtype=np.int32)
    changed = C.c_int64(0)
    check(lib.fnn_binary_morphology(labels_ptr, FNN_LABEL_U16 if uint16 else FNN_LABEL_U8, (C.c_int64 * 3)(*[int(i) for i in shape]),
                                    table.ctypes.data_as(C.POINTER(C.c_int32)), int(table.size), int(op), int(connectivity),
                                    int(iterations), int(border_value), int(background_label), int(fill_label), int(axes),
                                    C.byref(changed), stream), lib)
    return int(changed.value)


def confusion_counts(ref_ptr: int, pred_ptrs: Sequence[int], uint16: bool, n_vox: int, class_of_value, n_classes: int,
                     ignore_value: int = -1, stream: int = 0) -> np.ndarray:
    """fnn_confusion_counts on device label maps; returns int64 [n_pred, n_classes + 1, n_classes + 1]."""
    lib = load_library()
    table = np.ascontiguousarray(class_of_value, dtype=np.int32)
    n_pred = len(pred_ptrs)
    counts = np.zeros((max(n_pred, 1), int(n_classes) + 1, int(n_classes) + 1), np.int64)
    check(lib.fnn_confusion_counts(ref_ptr, (C.c_void_p * max(n_pred, 1))(*[int(p) for p in pred_ptrs]), n_pred,
                                   FNN_LABEL_U16 if uint16 else FNN_LABEL_U8, int(n_vox),
                                   table.ctypes.data_as(C.POINTER(C.c_int32)), int(table.size), int(n_classes),
                                   int(ignore_value), counts.ctypes.data_as(C.POINTER(C.c_int64)), stream), lib)
    return counts[:n_pred]


def _member_table(member):
    member = np.ascontiguousarray(member, dtype=np.uint8)
    if member.ndim != 2:
        raise ValueError('member must be [n_regions, n_table]')
    return member, member.ctypes.data_as(C.POINTER(C.c_uint8))


def surface_count(ref_ptr: int, pred_ptr: int, uint16: bool, shape, member, stream: int = 0):
    """fnn_surface_count on two device label maps (z, y, x); ``member`` uint8 [n_regions, n_table].  Returns
    (n_surface int64 [n_regions, 2] = surface voxels of ref and of pred, boxes int64 [n_regions, 6])."""
    lib = load_library()
    member, mp = _member_table(member)
    n_regions, n_table = member.shape
    n_surface = np.zeros((max(n_regions, 1), 2), np.int64)
    boxes = np.zeros((max(n_regions, 1), 6), np.int64)
    check(lib.fnn_surface_count(ref_ptr, pred_ptr, FNN_LABEL_U16 if uint16 else FNN_LABEL_U8,
                                (C.c_int64 * 3)(*[int(i) for i in shape]), mp, int(n_table), int(n_regions),
                                n_surface.ctypes.data_as(C.POINTER(C.c_int64)), boxes.ctypes.data_as(C.POINTER(C.c_int64)),
                                stream), lib)
    return n_surface[:n_regions], boxes[:n_regions]


def surface_distances(ref_ptr: int, pred_ptr: int, uint16: bool, shape, member, spacing, sq_dist_ptr: int, cap: int,
                      stream: int = 0) -> None:
    """fnn_surface_distances: the squared distances of every region with two non-empty sides into the device buffer of
    ``cap`` doubles at ``sq_dist_ptr``, in the order ``surface_count``'s sizes give (pred's surface, then ref's)."""
    lib = load_library()
    member, mp = _member_table(member)
    n_regions, n_table = member.shape
    check(lib.fnn_surface_distances(ref_ptr, pred_ptr, FNN_LABEL_U16 if uint16 else FNN_LABEL_U8,
                                    (C.c_int64 * 3)(*[int(i) for i in shape]), mp, int(n_table), int(n_regions),
                                    (C.c_double * 3)(*[float(s) for s in spacing]), sq_dist_ptr, int(cap), stream), lib)


def mesh_count(seg_ptr: int, uint16: bool, shape, member, stream: int = 0):
    """fnn_mesh_count on a device label map (z, y, x); ``member`` uint8 [n_regions, n_table].  Returns (counts int64
    [n_regions, 2] = vertices and faces of every region, boxes int64 [n_regions, 6])."""
    lib = load_library()
    member, mp = _member_table(member)
    n_regions, n_table = member.shape
    counts = np.zeros((max(n_regions, 1), 2), np.int64)
    boxes = np.zeros((max(n_regions, 1), 6), np.int64)
    check(lib.fnn_mesh_count(seg_ptr, FNN_LABEL_U16 if uint16 else FNN_LABEL_U8, (C.c_int64 * 3)(*[int(i) for i in shape]), mp,
                             int(n_table), int(n_regions), counts.ctypes.data_as(C.POINTER(C.c_int64)),
                             boxes.ctypes.data_as(C.POINTER(C.c_int64)), stream), lib)
    return counts[:n_regions], boxes[:n_regions]


def mesh_emit(seg_ptr: int, uint16: bool, shape, member, affine, smoothing_pairs: int, layout: int, points_ptr: int,
              cap_points: int, cells_ptr: int, cap_cells: int, cell_region_ptr: int, stream: int = 0) -> None:
    """fnn_mesh_emit: the points, triangles and triangle regions of every region into three device buffers with room for
    ``cap_points`` points and ``cap_cells`` triangles; ``affine`` 4x4 float64; layout 1: the bytes of a legacy-VTK file."""
    lib = load_library()
    member, mp = _member_table(member)
    n_regions, n_table = member.shape
    a = np.ascontiguousarray(affine, dtype=np.float64).reshape(16)
    check(lib.fnn_mesh_emit(seg_ptr, FNN_LABEL_U16 if uint16 else FNN_LABEL_U8, (C.c_int64 * 3)(*[int(i) for i in shape]), mp,
                            int(n_table), int(n_regions), (C.c_double * 16)(*a.tolist()), int(smoothing_pairs), int(layout),
                            points_ptr, int(cap_points), cells_ptr, int(cap_cells), cell_region_ptr, stream), lib)


def mesh_decimate(points_ptr: int, n: int, cells_ptr: int, cell_region_ptr: int, t: int, point_offsets, decimation_factor: float,
                  layout: int, out_points_ptr: int, cap_points: int, out_cells_ptr: int, cap_cells: int, out_cell_region_ptr: int,
                  stream: int = 0):
    """fnn_mesh_decimate on a layout-0 device model of ``n`` points and ``t`` triangles; ``point_offsets`` int64
    [n_regions + 1].  Returns (counts int64 [n_regions, 2] = points and triangles of every region, n_out, t_out, rounds,
    exhausted)."""
    lib = load_library()
    if not hasattr(lib, 'fnn_mesh_decimate'):
        raise EngineError(f'{LIB_PATH} has no fnn_mesh_decimate: rebuild the library')
    off = np.ascontiguousarray(point_offsets, dtype=np.int64).reshape(-1)
    n_regions = len(off) - 1
    counts = np.zeros((max(n_regions, 1), 2), np.int64)
    status = np.zeros(4, np.int64)
    P64 = C.POINTER(C.c_int64)
    check(lib.fnn_mesh_decimate(points_ptr, int(n), cells_ptr, cell_region_ptr, int(t), off.ctypes.data_as(P64), int(n_regions),
                                float(decimation_factor), int(layout), out_points_ptr, int(cap_points), out_cells_ptr, int(cap_cells),
                                out_cell_region_ptr, counts.ctypes.data_as(P64), status.ctypes.data_as(P64), stream), lib)
    return counts[:n_regions], int(status[0]), int(status[1]), int(status[2]), int(status[3])


INSTANCE_FIRST_CAPACITY = 65536        # records the first call of instance_overlaps has room for


def instance_overlaps_call(ref_ptr: int, pred_ptr: int, uint16: bool, shape, group_of_label, n_groups: int, records_ptr: int,
                           cap: int, stream: int = 0) -> np.ndarray:
    """One fnn_instance_overlaps call on two device label maps [X, Y, Z] with a device buffer of ``cap`` records of three
    int32 at ``records_ptr``.  Returns int64 (ref components, pred components, pieces); the buffer was written iff their sum
    is at most ``cap``."""
    lib = load_library()
    table = np.ascontiguousarray(group_of_label, dtype=np.int32)
    n_out = np.zeros(3, np.int64)
    check(lib.fnn_instance_overlaps(ref_ptr, pred_ptr, FNN_LABEL_U16 if uint16 else FNN_LABEL_U8,
                                    (C.c_int64 * 3)(*[int(i) for i in shape]), table.ctypes.data_as(C.POINTER(C.c_int32)),
                                    int(table.size), int(n_groups), records_ptr, int(cap),
                                    n_out.ctypes.data_as(C.POINTER(C.c_int64)), stream), lib)
    return n_out


def instance_overlaps(ref_ptr: int, pred_ptr: int, uint16: bool, shape, group_of_label, n_groups: int, stream: int = 0, *,
                      first_capacity: int = INSTANCE_FIRST_CAPACITY):
    """fnn_instance_overlaps with the record buffer owned here: a call with room for ``first_capacity`` records and, when
    that was short, one more with the exact size.  Returns (n_out int64 [3], records int32 [sum(n_out), 3] on the host, the
    number of calls made)."""
    import torch
    dev = torch.device('cuda', torch.cuda.current_device())
    cap, calls = max(int(first_capacity), 1), 0
    while True:
        buf = torch.empty(cap * 3, dtype=torch.int32, device=dev)
        n_out = instance_overlaps_call(ref_ptr, pred_ptr, uint16, shape, group_of_label, n_groups, buf.data_ptr(), cap, stream)
        calls += 1
        total = int(n_out.sum())
        if total <= cap:
            return n_out, buf[:total * 3].cpu().numpy().reshape(total, 3), calls
        if calls == 2:
            raise EngineError(f'fnn_instance_overlaps asked for {total} records after it was given {cap}')
        cap = total


def _order(regions_class_order, heads: int):
    if regions_class_order is None:
        return None
    assert len(regions_class_order) == heads
    return (C.c_int32 * heads)(*[int(c) for c in regions_class_order])


def ensemble_export(logits_ptrs: Sequence[int], halves: Sequence[bool], heads: int, regions_class_order, bbox,
                    shape_before_cropping, transpose_backward, avg_ptr: Optional[int], labels_ptr: int, uint16: bool,
                    stream: int = 0):
    """fnn_ensemble_export: the members' logits of the cropped grid (one device pointer each; fp16 where `halves`) ->
    average probabilities (skipped when avg_ptr is None) + labels on the original grid."""
    lib = load_library()
    n = len(logits_ptrs)
    assert len(halves) == n
    flat = (C.c_int64 * 6)(*[int(v) for ab in bbox for v in ab])
    check(lib.fnn_ensemble_export((C.c_void_p * max(n, 1))(*[int(p) for p in logits_ptrs]),
                                  (C.c_int32 * max(n, 1))(*[FNN_OUT_F16 if h else FNN_OUT_F32 for h in halves]), n, int(heads),
                                  _order(regions_class_order, heads), flat,
                                  (C.c_int64 * 3)(*[int(i) for i in shape_before_cropping]),
                                  (C.c_int32 * 3)(*[int(i) for i in transpose_backward]), avg_ptr, labels_ptr,
                                  FNN_LABEL_U16 if uint16 else FNN_LABEL_U8, stream), lib)


def ensemble_resample_export(members: Sequence[Tuple], heads: int, regions_class_order, bbox, shape_before_cropping,
                             transpose_backward, avg_ptr: Optional[int], labels_ptr: int, uint16: bool, stream: int = 0):
    """fnn_ensemble_resample_export: the members' logits on their own network grids - one ``(device pointer, half, shape[3],
    family, separate_axis or None)`` each - -> average probabilities (skipped when avg_ptr is None) + labels on the original
    grid, bit for bit those of ``resample`` (order 1, order_z 0) / ``resample_torch`` per member followed by
    ``ensemble_export``, without the resampled tensors.  A member whose shape equals the box's extents is taken as it is.
    op_last_kernels() names the kernel that ran."""
    lib = load_library()
    n = len(members)
    table = (EnsembleMember * max(n, 1))()
    for e, (ptr, half, shape, family, sep) in zip(table, members):
        e.logits, e.dtype, e.family = int(ptr), FNN_OUT_F16 if half else FNN_OUT_F32, int(family)
        e.shape = (C.c_int64 * 3)(*[int(i) for i in shape])
        e.separate_axis = -1 if sep is None else int(sep)
    flat = (C.c_int64 * 6)(*[int(v) for ab in bbox for v in ab])
    check(lib.fnn_ensemble_resample_export(table, n, int(heads), _order(regions_class_order, heads), flat,
                                           (C.c_int64 * 3)(*[int(i) for i in shape_before_cropping]),
                                           (C.c_int32 * 3)(*[int(i) for i in transpose_backward]), avg_ptr, labels_ptr,
                                           FNN_LABEL_U16 if uint16 else FNN_LABEL_U8, stream), lib)


def average_probabilities(probs_ptrs: Sequence[int], heads: int, regions_class_order, n_vox: int, avg_ptr: Optional[int],
                          labels_ptr: int, uint16: bool, stream: int = 0):
    """fnn_average_probabilities: float32 [heads, n_vox] device buffers -> average (skipped when avg_ptr is None) + labels."""
    lib = load_library()
    n = len(probs_ptrs)
    check(lib.fnn_average_probabilities((C.c_void_p * max(n, 1))(*[int(p) for p in probs_ptrs]), n, int(heads),
                                        _order(regions_class_order, heads), int(n_vox), avg_ptr, labels_ptr,
                                        FNN_LABEL_U16 if uint16 else FNN_LABEL_U8, stream), lib)


def op_conv3d(x, w, bias, k, stride, gamma=None, beta=None, slope=1.0, x2=None, gamma2=None, beta2=None, slope2=1.0,
              device=0, want_stats=False):
    """Single conv through the HIP kernel.  x [n,cin,D,H,W] float32 (host)."""
    lib = load_library()
    x = np.ascontiguousarray(x, np.float32)
    n, cin = x.shape[:2]
    dims = (C.c_int * 3)(*x.shape[2:])
    w = np.ascontiguousarray(w, np.float32)
    cout = w.shape[0]
    kk, ss = (C.c_int * 3)(*k), (C.c_int * 3)(*stride)
    od = [(x.shape[2 + i] + 2 * ((k[i] - 1) // 2) - k[i]) // stride[i] + 1 for i in range(3)]
    y = np.zeros((n, cout, *od), np.float32)
    stats = np.zeros((n, cout, 2), np.float64) if want_stats else None
    f = lambda a: None if a is None else np.ascontiguousarray(a, np.float32)
    x2, gamma, beta, gamma2, beta2, bias = f(x2), f(gamma), f(beta), f(gamma2), f(beta2), f(bias)
    rc = lib.fnn_op_conv3d(device, n, dims, _f32p(x), cin, _f32p(gamma), _f32p(beta), slope,
                           _f32p(x2), 0 if x2 is None else x2.shape[1], _f32p(gamma2), _f32p(beta2), slope2,
                           _f32p(w), _f32p(bias), cout, kk, ss, _f32p(y),
                           None if stats is None else stats.ctypes.data_as(C.POINTER(C.c_double)))
    check(rc, lib)
    return (y, stats) if want_stats else y


def op_conv_transpose3d(x, w, bias, stride, gamma=None, beta=None, slope=1.0, device=0):
    lib = load_library()
    x = np.ascontiguousarray(x, np.float32)
    n, cin = x.shape[:2]
    dims = (C.c_int * 3)(*x.shape[2:])
    w = np.ascontiguousarray(w, np.float32)
    cout = w.shape[1]
    ss = (C.c_int * 3)(*stride)
    y = np.zeros((n, cout, *[x.shape[2 + i] * stride[i] for i in range(3)]), np.float32)
    f = lambda a: None if a is None else np.ascontiguousarray(a, np.float32)
    gamma, beta, bias = f(gamma), f(beta), f(bias)
    rc = lib.fnn_op_conv_transpose3d(device, n, dims, _f32p(x), cin, _f32p(gamma), _f32p(beta), slope,
                                     _f32p(w), _f32p(bias), cout, ss, _f32p(y))
    check(rc, lib)
    return y


def _opt_f32(a):
    return None if a is None else np.ascontiguousarray(a, np.float32)


def _i3(v):
    return (C.c_int * 3)(*[int(i) for i in v])


def _u16p(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_uint16))


def op_avgpool(x, stride, gamma=None, beta=None, slope=1.0, x_cm=False, y_cm=False, device=0):
    """avgpool_kernel: AvgPool3d(stride, stride) of the transformed x [n,c,D,H,W] float32 (host) -> float32."""
    lib = load_library()
    x = np.ascontiguousarray(x, np.float32)
    n, c = x.shape[:2]
    gamma, beta = _opt_f32(gamma), _opt_f32(beta)
    y = np.zeros((n, c, *[x.shape[2 + i] // stride[i] for i in range(3)]), np.float32)
    check(lib.fnn_op_avgpool(device, n, _i3(x.shape[2:]), _f32p(x), c, _f32p(gamma), _f32p(beta), slope, _i3(stride),
                             int(x_cm), int(y_cm), _f32p(y)), lib)
    return y


def op_combine(a, b, slope, norm_a=None, slope_a=1.0, norm_b=None, slope_b=1.0, pool_stride=None, layouts=(0, 0, 0, 0), device=0):
    """combine_kernel / combine_pool_kernel: LeakyReLU(T_a(a) + T_b(b), slope) for a, b [n,c,D,H,W]; norm_* = (gamma, beta) or
    None; layouts = chunk-major flags of (a, b, out, pooled).  -> y, or (y, pooled) with a pool_stride."""
    lib = load_library()
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    assert a.shape == b.shape
    n, c = a.shape[:2]
    ga, ba = (_opt_f32(norm_a[0]), _opt_f32(norm_a[1])) if norm_a is not None else (None, None)
    gb, bb = (_opt_f32(norm_b[0]), _opt_f32(norm_b[1])) if norm_b is not None else (None, None)
    y = np.zeros(a.shape, np.float32)
    pooled = None if pool_stride is None else np.zeros((n, c, *[a.shape[2 + i] // pool_stride[i] for i in range(3)]), np.float32)
    check(lib.fnn_op_combine(device, n, _i3(a.shape[2:]), c, _f32p(a), _f32p(ga), _f32p(ba), slope_a,
                             _f32p(b), _f32p(gb), _f32p(bb), slope_b, slope, None if pool_stride is None else _i3(pool_stride),
                             *[int(v) for v in layouts], _f32p(y), _f32p(pooled)), lib)
    return y if pool_stride is None else (y, pooled)


INT_MAX = 2 ** 31 - 1


def op_seg_head(x, w, bias, item=0, mode=0, flips=(0, 0, 0), norm=None, slope=1.0, gauss_bits=None, acc=None, origin=(0, 0, 0),
                first_visit=None, patch_buf=None, device=0):
    """launch_head on item `item` of x [n,c,PD,PH,PW].  mode 0: acc [AX,Y,Z,HP] float16 or float32 is updated in place (a
    contiguous array); modes 1 / 2: patch_buf [heads, PD*PH*PW] float32 in place.  -> does the kernel honour first_visit."""
    lib = load_library()
    x = np.ascontiguousarray(x, np.float32)
    w = np.ascontiguousarray(w, np.float32)
    n, c = x.shape[:2]
    heads = w.shape[0]
    assert w.shape == (heads, c)
    g, bt = (_opt_f32(norm[0]), _opt_f32(norm[1])) if norm is not None else (None, None)
    bias = _opt_f32(bias)
    accp, fp32, box = None, 0, None
    if mode == 0:
        assert acc.flags['C_CONTIGUOUS'] and acc.dtype in (np.float16, np.float32) and acc.shape[3] == (heads + 1 + 7) // 8 * 8
        accp, fp32, box = acc.ctypes.data_as(C.c_void_p), int(acc.dtype == np.float32), (C.c_longlong * 3)(*acc.shape[:3])
    else:
        assert patch_buf.flags['C_CONTIGUOUS'] and patch_buf.dtype == np.float32 and patch_buf.shape == (heads, int(np.prod(x.shape[2:])))
    if gauss_bits is not None:
        gauss_bits = np.ascontiguousarray(gauss_bits, np.uint16).reshape(-1)
        assert gauss_bits.size == int(np.prod(x.shape[2:]))
    honoured = C.c_int(0)
    check(lib.fnn_op_seg_head(device, n, c, _i3(x.shape[2:]), _f32p(x), _f32p(g), _f32p(bt), slope, heads, _f32p(w), _f32p(bias),
                              int(item), int(mode), _i3(flips), _u16p(gauss_bits), accp, fp32, box, _i3(origin),
                              None if first_visit is None else _i3(first_visit), _f32p(patch_buf) if mode else None,
                              C.byref(honoured)), lib)
    return bool(honoured.value)


def op_patch_acc(patch_buf, patch, n_div, acc, origin=(0, 0, 0), gauss_bits=None, device=0):
    """patch_acc_kernel: acc [AX,Y,Z,HP] float16 / float32 (in place) += (patch_buf [heads, P] / n_div) * gaussian."""
    lib = load_library()
    patch_buf = np.ascontiguousarray(patch_buf, np.float32)
    heads = patch_buf.shape[0]
    assert acc.flags['C_CONTIGUOUS'] and acc.dtype in (np.float16, np.float32) and acc.shape[3] == (heads + 1 + 7) // 8 * 8
    assert patch_buf.shape[1] == int(np.prod(patch))
    if gauss_bits is not None:
        gauss_bits = np.ascontiguousarray(gauss_bits, np.uint16).reshape(-1)
        assert gauss_bits.size == patch_buf.shape[1]
    check(lib.fnn_op_patch_acc(device, _f32p(patch_buf), heads, _i3(patch), int(n_div), _u16p(gauss_bits),
                               acc.ctypes.data_as(C.c_void_p), int(acc.dtype == np.float32), (C.c_longlong * 3)(*acc.shape[:3]),
                               _i3(origin)), lib)


def op_patch_input(vol, origins, patch, cpad, flips=(0, 0, 0), chunk_major=False, device=0):
    """patch_input_kernel: vol [C,X,Y,Z] (one volume for every item) or [n,C,X,Y,Z] float32 -> uint16 fp16 bits [n,cpad,PD,PH,PW]."""
    lib = load_library()
    vol = np.ascontiguousarray(vol, np.float32)
    origins = np.ascontiguousarray(origins, np.int32).reshape(-1, 3)
    n = origins.shape[0]
    n_vol = 1 if vol.ndim == 4 else vol.shape[0]
    c = vol.shape[-4]
    out = np.zeros((n, cpad, *patch), np.uint16)
    check(lib.fnn_op_patch_input(device, _f32p(vol), n_vol, c, (C.c_longlong * 3)(*vol.shape[-3:]), n,
                                 origins.ctypes.data_as(C.POINTER(C.c_int)), _i3(flips), _i3(patch), int(cpad), int(chunk_major),
                                 _u16p(out)), lib)
    return out


FUSE_STEM, FUSE_TCONV = 1, 2


def _f64p(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))


def op_stem(vol, origins, patch, w, bias, flips=(0, 0, 0), want_stats=False, device=0):
    """launch_stem_mfma on patch windows of vol [C,X,Y,Z] (one volume for every item) or [n,C,X,Y,Z] float32 at origins [n,3]:
    w [cout,C,kd,kh,kw] -> y [n,cout,*patch] float32 (and the statistics [n,cout,2])."""
    lib = load_library()
    vol = np.ascontiguousarray(vol, np.float32)
    origins = np.ascontiguousarray(origins, np.int32).reshape(-1, 3)
    w, bias = np.ascontiguousarray(w, np.float32), _opt_f32(bias)
    n, n_vol, c, cout = origins.shape[0], 1 if vol.ndim == 4 else vol.shape[0], vol.shape[-4], w.shape[0]
    assert w.shape[1] == c
    y = np.zeros((n, cout, *patch), np.float32)
    stats = np.zeros((n, cout, 2), np.float64) if want_stats else None
    check(lib.fnn_op_stem(device, _f32p(vol), n_vol, c, (C.c_longlong * 3)(*vol.shape[-3:]), n,
                          origins.ctypes.data_as(C.POINTER(C.c_int)), _i3(flips), _i3(patch), _f32p(w), _f32p(bias), cout,
                          _i3(w.shape[2:]), _f32p(y), _f64p(stats)), lib)
    return (y, stats) if want_stats else y


def op_conv_fused_stem(vol, origins, patch, stem_w, stem_bias, stem_norm, stem_slope, w, bias, flips=(0, 0, 0), device=0):
    """fnn_op_conv_fused, mode FUSE_STEM: vol [1,X,Y,Z] or [n,1,X,Y,Z]; stem_w [16,1,*k], stem_norm = (gamma, beta); w [16,16,*k]
    -> (y [n,16,*patch], statistics [n,16,2])."""
    lib = load_library()
    vol = np.ascontiguousarray(vol, np.float32)
    origins = np.ascontiguousarray(origins, np.int32).reshape(-1, 3)
    stem_w, w = np.ascontiguousarray(stem_w, np.float32), np.ascontiguousarray(w, np.float32)
    stem_bias, bias, g, b = _opt_f32(stem_bias), _opt_f32(bias), _opt_f32(stem_norm[0]), _opt_f32(stem_norm[1])
    n, n_vol = origins.shape[0], 1 if vol.ndim == 4 else vol.shape[0]
    assert vol.shape[-4] == 1 and stem_w.shape[:2] == (16, 1) and w.shape[:2] == (16, 16) and stem_w.shape[2:] == w.shape[2:]
    y, stats = np.zeros((n, 16, *patch), np.float32), np.zeros((n, 16, 2), np.float64)
    check(lib.fnn_op_conv_fused(device, FUSE_STEM, n, _i3(patch), _f32p(vol), n_vol, (C.c_longlong * 3)(*vol.shape[-3:]),
                                origins.ctypes.data_as(C.POINTER(C.c_int)), _i3(flips), None, 0, None, None, None, None, 1.0,
                                _f32p(stem_w), _f32p(stem_bias), _f32p(g), _f32p(b), stem_slope, _f32p(w), _f32p(bias),
                                _i3(w.shape[2:]), _f32p(y), _f64p(stats)), lib)
    return y, stats


def op_conv_fused_tconv(low, low_norm, low_slope, tw, tbias, tstride, skip, skip_norm, skip_slope, w, bias, device=0):
    """fnn_op_conv_fused, mode FUSE_TCONV: low [n,16|32,Dl,Hl,Wl] (norm = (gamma, beta) or None), tw [low_c,16,*tstride];
    skip [n,16,D,H,W]; w [16,32,1,3,3] over (up, skip) -> (y [n,16,D,H,W], statistics [n,16,2])."""
    lib = load_library()
    low, skip = np.ascontiguousarray(low, np.float32), np.ascontiguousarray(skip, np.float32)
    tw, w = np.ascontiguousarray(tw, np.float32), np.ascontiguousarray(w, np.float32)
    tbias, bias = _opt_f32(tbias), _opt_f32(bias)
    lg, lb = (_opt_f32(low_norm[0]), _opt_f32(low_norm[1])) if low_norm is not None else (None, None)
    sg, sb = (_opt_f32(skip_norm[0]), _opt_f32(skip_norm[1])) if skip_norm is not None else (None, None)
    n, low_c = low.shape[:2]
    dims = skip.shape[2:]
    assert tuple(dims) == tuple(low.shape[2 + i] * tstride[i] for i in range(3)) and skip.shape[:2] == (n, 16)
    assert tw.shape == (low_c, 16, *tstride) and w.shape[:2] == (16, 32)
    y, stats = np.zeros((n, 16, *dims), np.float32), np.zeros((n, 16, 2), np.float64)
    check(lib.fnn_op_conv_fused(device, FUSE_TCONV, n, _i3(dims), None, 0, None, None, None, _f32p(low), low_c, _i3(tstride),
                                _f32p(skip), _f32p(sg), _f32p(sb), skip_slope, _f32p(tw), _f32p(tbias), _f32p(lg), _f32p(lb),
                                low_slope, _f32p(w), _f32p(bias), _i3(w.shape[2:]), _f32p(y), _f64p(stats)), lib)
    return y, stats


def op_last_kernels():
    """Kernel variants launched by this thread's last op_* (or resample_labels) call."""
    lib = load_library()
    buf = C.create_string_buffer(4096)
    lib.fnn_op_last_kernels(buf, 4096)
    return [k for k in buf.value.decode().split('\n') if k]


def clock_probe_start(device=0, max_seconds=1.0):
    """One sleeping wave that reads the shader-clock and the 100 MHz counters for max_seconds or until clock_probe_stop (include/fnn.h)."""
    lib = load_library()
    h = C.c_void_p()
    check(lib.fnn_clock_probe_start(device, float(max_seconds), C.byref(h)), lib)
    return h


def clock_probe_stop(handle):
    """(GHz the device held since clock_probe_start, seconds covered)."""
    lib = load_library()
    ghz, sec = C.c_double(), C.c_double()
    check(lib.fnn_clock_probe_stop(handle, C.byref(ghz), C.byref(sec)), lib)
    return ghz.value, sec.value


def op_quotient_check(device=0):
    """(differing pairs, pairs on the fast route, (a bits, b bits) of one differing pair) of the gather epilogue's quotient over all fp16 a, b >= +0."""
    lib = load_library()
    counts = (C.c_uint64 * 3)()
    check(lib.fnn_op_quotient_check(device, counts), lib)
    return int(counts[0]), int(counts[1]), (int(counts[2]) & 0xFFFF, int(counts[2]) >> 16)


class Engine:
    """Thin RAII wrapper around an ``fnn_engine*``."""

    def __init__(self, desc: ArchDesc, device: int = 0, max_batch: int = 4):
        self.lib = load_library()
        self.handle = C.c_void_p()
        self.desc = desc
        check(self.lib.fnn_create(C.byref(desc), int(device), int(max_batch), C.byref(self.handle)), self.lib, None)
        self.max_batch = max_batch
        self.device = device

    def close(self):
        if getattr(self, 'handle', None) is not None and self.handle:
            self.lib.fnn_destroy(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def weight_count(self) -> int:
        return int(self.lib.fnn_weight_count(self.handle))

    def load_weights(self, fold: int, blob: np.ndarray):
        blob = np.ascontiguousarray(blob, np.float32)
        check(self.lib.fnn_load_weights(self.handle, fold, blob.ctypes.data, blob.size), self.lib, self.handle)

    def set_gaussian(self, half_bits: np.ndarray):
        hb = np.ascontiguousarray(half_bits, np.uint16)
        check(self.lib.fnn_set_gaussian(self.handle, hb.ctypes.data, hb.size), self.lib, self.handle)

    def set_profiling(self, on: bool):
        check(self.lib.fnn_set_profiling(self.handle, int(on)), self.lib, self.handle)

    def profile(self) -> Profile:
        p = Profile()
        check(self.lib.fnn_get_profile(self.handle, C.byref(p)), self.lib, self.handle)
        return p

    def kernel_log(self):
        """Kernel variants of the last call made with profiling on, one per launch."""
        n = self.lib.fnn_kernel_log(self.handle, None, 0)
        buf = C.create_string_buffer(int(n))
        self.lib.fnn_kernel_log(self.handle, buf, n)
        return [k for k in buf.value.decode().split('\n') if k]

    def _text(self, fn):
        n = fn(self.handle, None, 0)
        buf = C.create_string_buffer(int(n))
        fn(self.handle, buf, n)
        return [r.split('\t') for r in buf.value.decode().split('\n') if r]

    def profile_launches(self):
        """Rows (layer, family, ms, flops, bytes, kernels) of every timed launch of the last profiled call."""
        return [(int(r[0]), r[1], float(r[2]), float(r[3]), float(r[4]), r[5] if len(r) > 5 else '') for r in self._text(self.lib.fnn_profile_launches)]

    def layer_table(self):
        """The engine's layer plan: dicts with index, type, cin, cout, kernel, stride, in_dims, out_dims, flops, bytes, fused and
        picked - the kernel chosen for a conv layer, as kernel_log() names it ('-' for other layers)."""
        return _layer_rows(self._text(self.lib.fnn_layer_table))

    def patch_work(self):
        fl, by = C.c_double(), C.c_double()
        check(self.lib.fnn_patch_work(self.handle, C.byref(fl), C.byref(by)), self.lib, self.handle)
        return fl.value, by.value

    def predict_volume(self, vol_ptr: int, shape, opts: Opts, out_ptr: int, fold: int = 0, n_folds: int = 0):
        shp = (C.c_int64 * 4)(*[int(i) for i in shape])
        if n_folds > 0:
            rc = self.lib.fnn_predict_volume_ensemble(self.handle, n_folds, vol_ptr, shp, C.byref(opts), out_ptr)
        else:
            rc = self.lib.fnn_predict_volume(self.handle, fold, vol_ptr, shp, C.byref(opts), out_ptr)
        check(rc, self.lib, self.handle)

    def predict_labels(self, vol_ptr: int, shape, opts: Opts, labels_ptr: int, n_folds: int = 1):
        shp = (C.c_int64 * 4)(*[int(i) for i in shape])
        check(self.lib.fnn_predict_labels(self.handle, n_folds, vol_ptr, shp, C.byref(opts), labels_ptr),
              self.lib, self.handle)

    @property
    def accumulator_channels(self) -> int:
        return int(self.lib.fnn_accumulator_channels(self.handle))

    def accumulate_patches(self, vol_ptr, shape, opts, patch_ids, box_lo, box_hi, acc_ptr, fold=0):
        shp = (C.c_int64 * 4)(*[int(i) for i in shape])
        ids = (C.c_int64 * max(1, len(patch_ids)))(*[int(i) for i in patch_ids])
        lo, hi = (C.c_int64 * 3)(*[int(i) for i in box_lo]), (C.c_int64 * 3)(*[int(i) for i in box_hi])
        check(self.lib.fnn_accumulate_patches(self.handle, fold, vol_ptr, shp, C.byref(opts), ids, len(patch_ids),
                                              lo, hi, acc_ptr), self.lib, self.handle)

    def normalize_box(self, acc_ptr, shape, opts, box_lo, box_hi, out_lo, out_hi, out_ptr):
        shp = (C.c_int64 * 4)(*[int(i) for i in shape])
        a = [(C.c_int64 * 3)(*[int(i) for i in v]) for v in (box_lo, box_hi, out_lo, out_hi)]
        check(self.lib.fnn_normalize_box(self.handle, acc_ptr, shp, C.byref(opts), a[0], a[1], a[2], a[3], out_ptr),
              self.lib, self.handle)

    @property
    def feature_channels(self) -> int:
        return int(self.lib.fnn_feature_channels(self.handle))

    def patch_features(self, vol_ptr, shape, opts, patch_ids, feat_ptr, fss_ptr, fold=0, slot0=0, n_slots=None):
        """feat [n_eval][n_slots][P][C] / fss [n_eval][n_slots][2][C] (base pointers): patch_ids[i] -> slot slot0 + i."""
        shp = (C.c_int64 * 4)(*[int(i) for i in shape])
        ids = (C.c_int64 * max(1, len(patch_ids)))(*[int(i) for i in patch_ids])
        n_slots = slot0 + len(patch_ids) if n_slots is None else n_slots
        check(self.lib.fnn_patch_features(self.handle, fold, vol_ptr, shp, C.byref(opts), ids, len(patch_ids), feat_ptr, fss_ptr,
                                          C.c_int64(slot0), C.c_int64(n_slots)), self.lib, self.handle)

    def gather_box(self, feat_ptr, fss_ptr, slot_of_patch, shape, opts, out_lo, out_hi, logits_ptr=None, labels_ptr=None, fold=0,
                   n_slots=None):
        shp = (C.c_int64 * 4)(*[int(i) for i in shape])
        tab = np.ascontiguousarray(slot_of_patch, np.int32)
        n_slots = int(tab.max()) + 1 if n_slots is None else n_slots
        lo, hi = (C.c_int64 * 3)(*[int(i) for i in out_lo]), (C.c_int64 * 3)(*[int(i) for i in out_hi])
        check(self.lib.fnn_gather_box(self.handle, fold, feat_ptr, fss_ptr, tab.ctypes.data_as(C.POINTER(C.c_int32)),
                                      C.c_int64(max(1, n_slots)), shp, C.byref(opts), lo, hi, logits_ptr, labels_ptr),
              self.lib, self.handle)

    def pack_regions(self, feat_ptr, n_slots, regions_ptr, n, message_ptr, stream=0):
        """`n` sub-blocks of the kept activations (device table of fnn_region records, include/fnn.h) -> one message buffer."""
        check(self.lib.fnn_pack_regions(self.handle, feat_ptr, C.c_int64(n_slots), regions_ptr, C.c_int64(n), message_ptr, stream),
              self.lib, self.handle)

    def unpack_regions(self, feat_ptr, n_slots, regions_ptr, n, message_ptr, stream=0):
        check(self.lib.fnn_unpack_regions(self.handle, feat_ptr, C.c_int64(n_slots), regions_ptr, C.c_int64(n), message_ptr, stream),
              self.lib, self.handle)

    def labels_box(self, acc_ptr, shape, opts, box_lo, box_hi, out_lo, out_hi, labels_ptr):
        shp = (C.c_int64 * 4)(*[int(i) for i in shape])
        a = [(C.c_int64 * 3)(*[int(i) for i in v]) for v in (box_lo, box_hi, out_lo, out_hi)]
        check(self.lib.fnn_labels_box(self.handle, acc_ptr, shp, C.byref(opts), a[0], a[1], a[2], a[3], labels_ptr),
              self.lib, self.handle)

    def forward_patches(self, x_ptr: int, n: int, out_ptr: int, fold: int = 0, stream: int = 0):
        check(self.lib.fnn_forward_patches(self.handle, fold, x_ptr, n, out_ptr, stream), self.lib, self.handle)

    def set_label_rule(self, regions_class_order=None, uint16: bool = False):
        """``None`` = argmax over heads; a sequence = region-based training (sigmoid > 0.5 painted in that order)."""
        dt = FNN_LABEL_U16 if uint16 else FNN_LABEL_U8
        if regions_class_order is None:
            rc = self.lib.fnn_set_label_rule(self.handle, FNN_LABELS_ARGMAX, None, 0, dt)
        else:
            order = (C.c_int32 * len(regions_class_order))(*[int(i) for i in regions_class_order])
            rc = self.lib.fnn_set_label_rule(self.handle, FNN_LABELS_REGIONS, order, len(regions_class_order), dt)
        check(rc, self.lib, self.handle)

    def argmax_labels(self, logits_ptr, dtype, heads, n_vox, labels_ptr, stream=0):
        check(self.lib.fnn_argmax_labels(self.handle, logits_ptr, dtype, heads, n_vox, labels_ptr, stream),
              self.lib, self.handle)
