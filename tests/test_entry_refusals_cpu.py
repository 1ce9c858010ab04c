"""What the file-level entry points (prep, resample, resample_torch, export_labels, postprocess, ensemble, metrics, imageio,
reorient, deflate, deflate_masks) refuse before they touch the device: a table of bad calls through the C ABI with the
return code and the exact fnn_last_error(NULL) text of each.  No machine without a GPU owns device memory, so every call ends
at the latest at the entry's device-pointer refusal; what lies behind that one (the crop-box checks of fnn_preprocess,
fnn_revert_labels and fnn_export_probabilities) is pinned on the GPU in tests/test_gpu_prep_ops.py.  The texts were recorded
from the library before the entries' host prologues were shared, and must stay what they were."""
import ctypes as C

import numpy as np
import pytest

from fast_nnunet_amd import capi

INVALID, UNSUPPORTED = capi.FNN_E_INVALID, capi.FNN_E_UNSUPPORTED
U8, U16, F16, F32 = capi.FNN_LABEL_U8, capi.FNN_LABEL_U16, capi.FNN_OUT_F16, capi.FNN_OUT_F32

_HOST = np.zeros(1 << 16, np.uint8)
_BASE = (_HOST.ctypes.data + 63) & ~63          # host memory, 64-byte aligned


def hp(off=0):
    return C.c_void_p(_BASE + off)


def i64(*v):
    return (C.c_int64 * len(v))(*v)


def i32(*v):
    return (C.c_int32 * len(v))(*v)


def ptrs(*v):
    return (C.c_void_p * len(v))(*v)


def norm(*schemes):
    a = (capi.NormDesc * len(schemes))()
    for d, s in zip(a, schemes):
        d.scheme, d.mean, d.std, d.lower, d.upper, d.use_mask = s, 0.0, 1.0, -1.0, 1.0, 0
    return a


def rdesc(order=3, sep=-1, order_z=0, dtype=F32):
    return C.pointer(capi.ResampleDesc(order, sep, order_z, dtype))


def tdesc(dtype=F32, sep=-1, memeff=0, mode=capi.FNN_INTERP_LINEAR, aniso=capi.FNN_INTERP_NEAREST_EXACT):
    return C.pointer(capi.ResampleTorchDesc(dtype, sep, memeff, mode, aniso))


NULL = None
S4, S3, ID, BOX = i64(1, 4, 4, 4), i64(4, 4, 4), i32(0, 1, 2), i64(0, 4, 0, 4, 0, 4)
BAD_PERMS = {'repeated': i32(0, 1, 1), 'out_of_range': i32(0, 1, 3), 'negative': i32(-1, 1, 2)}
OUT6, O64, O32, OU32 = i64(*[0] * 6), i64(*[0] * 64), i32(0), (C.c_uint32 * 4)()
DEV = ' needs device pointers (no CPU path)'
PERM_TF = 'transpose_forward is not a permutation of (0, 1, 2)'
PERM_TB = 'transpose_backward is not a permutation of (0, 1, 2)'
BBOX_BEFORE = 'bbox outside shape_before_cropping'
NIFTI = ': NIfTI datatype not served (uint8, int8, int16, uint16, int32, uint32, float32 and float64 are)'


def _with(args, k, v):
    return args[:k] + (v,) + args[k + 1:]


def _nulls(fn, good, which, code, msg):
    return [(f'{fn}-null-{k}', fn, _with(good, k, NULL), code, msg) for k in which]


def _rows():
    R = []
    # ---- prep.hip
    g = (hp(), S4, ID, OUT6, NULL)
    R += _nulls('fnn_nonzero_bbox', g, range(4), INVALID, 'NULL argument')
    R += [(f'fnn_nonzero_bbox-perm-{n}', 'fnn_nonzero_bbox', _with(g, 2, p), INVALID, PERM_TF) for n, p in BAD_PERMS.items()]
    R += [(f'fnn_nonzero_bbox-shape-{n}', 'fnn_nonzero_bbox', _with(g, 1, s), INVALID, 'bad shape (1..8 channels)')
          for n, s in {'c0': i64(0, 4, 4, 4), 'c9': i64(9, 4, 4, 4), 'x0': i64(1, 0, 4, 4), 'z0': i64(1, 4, 4, 0)}.items()]
    R += [('fnn_nonzero_bbox-host', 'fnn_nonzero_bbox', g, INVALID, 'fnn_nonzero_bbox needs a device pointer (no CPU path)')]
    g = (hp(), S4, ID, BOX, norm(capi.FNN_NORM_ZSCORE), hp(4096), NULL)
    R += _nulls('fnn_preprocess', g, range(6), INVALID, 'NULL argument')
    R += [(f'fnn_preprocess-perm-{n}', 'fnn_preprocess', _with(g, 2, p), INVALID, PERM_TF) for n, p in BAD_PERMS.items()]
    R += [('fnn_preprocess-c0', 'fnn_preprocess', _with(g, 1, i64(0, 4, 4, 4)), INVALID, '1..8 channels'),
          ('fnn_preprocess-c9', 'fnn_preprocess', _with(g, 1, i64(9, 4, 4, 4)), INVALID, '1..8 channels'),
          ('fnn_preprocess-host', 'fnn_preprocess', g, INVALID, 'fnn_preprocess' + DEV),
          # behind the pointer check on purpose: neither an unknown scheme nor a bad box is looked at for host memory
          ('fnn_preprocess-unknown-scheme-host', 'fnn_preprocess', _with(g, 4, norm(77)), INVALID, 'fnn_preprocess' + DEV),
          ('fnn_preprocess-bbox-host', 'fnn_preprocess', _with(g, 3, i64(0, 5, 0, 4, 0, 4)), INVALID, 'fnn_preprocess' + DEV)]
    g = (hp(), U8, BOX, S3, ID, hp(4096), NULL)
    R += _nulls('fnn_revert_labels', g, (0, 2, 3, 4, 5), INVALID, 'NULL argument')
    R += [(f'fnn_revert_labels-perm-{n}', 'fnn_revert_labels', _with(g, 4, p), INVALID, PERM_TB) for n, p in BAD_PERMS.items()]
    R += [('fnn_revert_labels-dtype', 'fnn_revert_labels', _with(g, 1, 2), INVALID, 'unknown label dtype'),
          ('fnn_revert_labels-host', 'fnn_revert_labels', g, INVALID, 'fnn_revert_labels' + DEV),
          ('fnn_revert_labels-bbox-host', 'fnn_revert_labels', _with(g, 2, i64(0, 5, 0, 4, 0, 4)), INVALID, 'fnn_revert_labels' + DEV)]
    g = (hp(), F16, 2, NULL, BOX, S3, ID, hp(4096), hp(8192), U8, NULL)
    R += _nulls('fnn_export_probabilities', g, (0, 4, 5, 6, 7, 8), INVALID, 'NULL argument')
    R += [(f'fnn_export_probabilities-perm-{n}', 'fnn_export_probabilities', _with(g, 6, p), INVALID, PERM_TB) for n, p in BAD_PERMS.items()]
    R += [('fnn_export_probabilities-label-dtype', 'fnn_export_probabilities', _with(g, 9, -1), INVALID, 'unknown label dtype'),
          ('fnn_export_probabilities-logits-dtype', 'fnn_export_probabilities', _with(g, 1, 2), INVALID, 'unknown logits dtype'),
          ('fnn_export_probabilities-heads0', 'fnn_export_probabilities', _with(g, 2, 0), INVALID, 'bad number of heads'),
          ('fnn_export_probabilities-heads4097', 'fnn_export_probabilities', _with(g, 2, 4097), INVALID, 'bad number of heads'),
          ('fnn_export_probabilities-host', 'fnn_export_probabilities', g, INVALID, 'fnn_export_probabilities' + DEV),
          ('fnn_export_probabilities-bbox-host', 'fnn_export_probabilities', _with(g, 4, i64(2, 2, 0, 4, 0, 4)), INVALID,
           'fnn_export_probabilities' + DEV)]
    # ---- resample.hip
    g = (hp(), S4, S3, rdesc(), hp(4096), NULL)
    R += _nulls('fnn_resample', g, range(5), INVALID, 'NULL argument')
    R += [('fnn_resample-order2', 'fnn_resample', _with(g, 3, rdesc(order=2)), UNSUPPORTED, 'interpolation order must be 0, 1 or 3'),
          ('fnn_resample-sep3', 'fnn_resample', _with(g, 3, rdesc(sep=3)), INVALID, 'separate_axis must be -1 .. 2'),
          ('fnn_resample-sep-2', 'fnn_resample', _with(g, 3, rdesc(sep=-2)), INVALID, 'separate_axis must be -1 .. 2'),
          ('fnn_resample-order_z', 'fnn_resample', _with(g, 3, rdesc(sep=0, order_z=1)), UNSUPPORTED, 'order_z other than 0 is not implemented'),
          ('fnn_resample-dtype', 'fnn_resample', _with(g, 3, rdesc(dtype=2)), INVALID, 'unknown dtype'),
          ('fnn_resample-shape', 'fnn_resample', _with(g, 1, i64(1, 4, 0, 4)), INVALID, 'bad shape'),
          ('fnn_resample-new_shape', 'fnn_resample', _with(g, 2, i64(4, 4, 0)), INVALID, 'bad new_shape'),
          ('fnn_resample-host', 'fnn_resample', g, INVALID, 'fnn_resample' + DEV)]
    # ---- resample_torch.hip
    for fn in ('fnn_resample_torch', 'fnn_resample_torch_seg'):
        g = (hp(), S4, S3, tdesc(), hp(4096), NULL)
        R += _nulls(fn, g, range(5), INVALID, 'NULL argument')
        R += [(fn + '-mode', fn, _with(g, 3, tdesc(mode=capi.FNN_INTERP_OTHER)), UNSUPPORTED, "mode other than 'linear' is not implemented"),
              (fn + '-aniso', fn, _with(g, 3, tdesc(aniso=capi.FNN_INTERP_LINEAR)), UNSUPPORTED,
               "aniso_axis_mode other than 'nearest-exact' is not implemented"),
              (fn + '-sep3', fn, _with(g, 3, tdesc(sep=3)), INVALID, 'separate_axis must be -1 .. 2'),
              (fn + '-shape', fn, _with(g, 1, i64(0, 4, 4, 4)), INVALID, 'bad shape'),
              (fn + '-new_shape', fn, _with(g, 2, i64(4, 0, 4)), INVALID, 'bad new_shape'),
              (fn + '-host', fn, g, INVALID, 'the torch resampling kernels need device pointers (no CPU path)'),
              # the float dtype of the image entry is looked at after the pointers
              (fn + '-dtype-host', fn, _with(g, 3, tdesc(dtype=2)), INVALID, 'the torch resampling kernels need device pointers (no CPU path)')]
    # ---- export_labels.hip
    fn = 'fnn_resample_labels'
    g = (hp(), F16, i64(2, 4, 4, 4), S3, capi.FNN_RESAMPLE_TORCH, -1, NULL, 0, hp(4096), U8, NULL)
    R += _nulls(fn, g, (0, 2, 3, 8), INVALID, 'NULL argument')
    R += [(fn + '-family', fn, _with(g, 4, 2), UNSUPPORTED, 'unknown resampling family'),
          (fn + '-dtype', fn, _with(g, 1, 2), INVALID, 'unknown dtype'),
          (fn + '-label-dtype', fn, _with(g, 9, 2), INVALID, 'unknown label dtype'),
          (fn + '-sep3', fn, _with(g, 5, 3), INVALID, 'separate_axis must be -1 .. 2'),
          (fn + '-heads0', fn, _with(g, 2, i64(0, 4, 4, 4)), INVALID, 'heads must be at least 1'),
          (fn + '-shape', fn, _with(g, 2, i64(2, 4, 4, 0)), INVALID, 'bad shape'),
          (fn + '-new_shape', fn, _with(g, 3, i64(0, 4, 4)), INVALID, 'bad new_shape'),
          (fn + '-regions-count', fn, _with(_with(g, 6, hp(8192)), 7, 3), INVALID, 'regions_class_order needs one entry per head'),
          (fn + '-257-heads-u8', fn, _with(g, 2, i64(257, 4, 4, 4)), INVALID, 'more than 256 heads need uint16 labels'),
          (fn + '-host', fn, g, INVALID, fn + DEV),
          (fn + '-host-order', fn, _with(_with(g, 6, hp(8192)), 7, 2), INVALID, fn + DEV)]
    # ---- postprocess.hip
    fn = 'fnn_keep_largest_components'
    g = (hp(), U8, S3, i32(-1, 0, 0), 3, 1, 0, NULL, NULL)
    R += [(fn + '-null-shape', fn, _with(g, 2, NULL), INVALID, 'NULL shape'),
          (fn + '-dtype', fn, _with(g, 1, 2), INVALID, 'unknown label dtype'),
          (fn + '-background-256-u8', fn, _with(g, 6, 256), INVALID, 'background_label outside the label dtype'),
          (fn + '-background-negative', fn, _with(g, 6, -1), INVALID, 'background_label outside the label dtype'),
          (fn + '-negative-shape', fn, _with(g, 2, i64(4, -1, 4)), INVALID, 'negative shape'),
          (fn + '-negative-groups', fn, _with(g, 5, -1), INVALID, 'bad label-set table'),
          (fn + '-null-table', fn, _with(g, 3, NULL), INVALID, 'bad label-set table'),
          (fn + '-table-entry', fn, _with(g, 3, i32(-1, 1, 0)), INVALID, 'group_of_label entry outside [-1, n_groups)'),
          (fn + '-too-large', fn, _with(g, 2, i64(2048, 2048, 1024)), UNSUPPORTED, fn + ': more than 2^31 - 1 voxels'),
          (fn + '-null-labels', fn, _with(g, 0, NULL), INVALID, fn + ' needs a device label map (no CPU path)'),
          (fn + '-host', fn, g, INVALID, fn + ' needs a device label map (no CPU path)')]
    # ---- ensemble.hip
    fn = 'fnn_ensemble_export'
    g = (ptrs(_BASE, _BASE + 4096), i32(F16, F32), 2, 2, NULL, BOX, S3, ID, NULL, hp(8192), U8, NULL)
    R += _nulls(fn, g, (0, 1, 5, 6, 7, 9), INVALID, 'NULL argument')
    R += [(fn + '-members0', fn, _with(g, 2, 0), INVALID, 'n_members must be 1..16'),
          (fn + '-members17', fn, _with(g, 2, 17), INVALID, 'n_members must be 1..16'),
          (fn + '-null-member', fn, _with(g, 0, ptrs(_BASE, None)), INVALID, 'NULL member logits'),
          (fn + '-member-dtype', fn, _with(g, 1, i32(F16, 2)), INVALID, 'unknown member logits dtype'),
          (fn + '-heads0', fn, _with(g, 3, 0), INVALID, 'bad number of heads'),
          (fn + '-label-dtype', fn, _with(g, 10, 2), INVALID, 'unknown label dtype'),
          (fn + '-bbox-hi', fn, _with(g, 5, i64(0, 4, 0, 5, 0, 4)), INVALID, BBOX_BEFORE),
          (fn + '-bbox-negative', fn, _with(g, 5, i64(-1, 4, 0, 4, 0, 4)), INVALID, BBOX_BEFORE),
          (fn + '-bbox-empty', fn, _with(g, 5, i64(0, 4, 0, 4, 3, 3)), INVALID, BBOX_BEFORE),
          (fn + '-host', fn, g, INVALID, fn + DEV)]
    R += [(f'{fn}-perm-{n}', fn, _with(g, 7, p), INVALID, PERM_TB) for n, p in BAD_PERMS.items()]
    fn = 'fnn_average_probabilities'
    g = (ptrs(_BASE, _BASE + 4096), 2, 2, NULL, 64, NULL, hp(8192), U8, NULL)
    R += _nulls(fn, g, (0, 6), INVALID, 'NULL argument')
    R += [(fn + '-members0', fn, _with(g, 1, 0), INVALID, 'n_members must be 1..16'),
          (fn + '-null-member', fn, _with(g, 0, ptrs(None, _BASE)), INVALID, 'NULL member probabilities'),
          (fn + '-heads4097', fn, _with(g, 2, 4097), INVALID, 'bad number of heads'),
          (fn + '-label-dtype', fn, _with(g, 7, -1), INVALID, 'unknown label dtype'),
          (fn + '-negative-n_vox', fn, _with(g, 4, -1), INVALID, 'negative n_vox'),
          (fn + '-host', fn, g, INVALID, fn + DEV)]
    # ---- metrics.hip
    fn = 'fnn_confusion_counts'
    g = (hp(), ptrs(_BASE + 4096), 1, U8, 64, i32(0, 1), 2, 2, -1, O64, NULL)
    MAPS = fn + ' needs device label maps (no CPU path)'
    R += [(fn + '-dtype', fn, _with(g, 3, 2), INVALID, 'unknown label dtype'),
          (fn + '-n_pred0', fn, _with(g, 2, 0), INVALID, fn + ': n_pred must be 1..4'),
          (fn + '-n_pred5', fn, _with(g, 2, 5), INVALID, fn + ': n_pred must be 1..4'),
          (fn + '-classes256', fn, _with(g, 7, 256), INVALID, fn + ': n_classes must be 0..255'),
          (fn + '-negative-n_vox', fn, _with(g, 4, -1), INVALID, 'negative voxel count'),
          (fn + '-null-table', fn, _with(g, 5, NULL), INVALID, 'bad class table'),
          (fn + '-negative-table', fn, _with(g, 6, -1), INVALID, 'bad class table'),
          (fn + '-null-counts', fn, _with(g, 9, NULL), INVALID, 'NULL pred or counts'),
          (fn + '-null-pred', fn, _with(g, 1, NULL), INVALID, 'NULL pred or counts'),
          (fn + '-table-entry', fn, _with(g, 5, i32(0, 2)), INVALID, 'class_of_value entry outside [-1, n_classes)'),
          (fn + '-null-ref', fn, _with(g, 0, NULL), INVALID, MAPS),
          (fn + '-host', fn, g, INVALID, MAPS),
          (fn + '-misaligned-host', fn, _with(g, 0, hp(8)), INVALID, MAPS)]
    # ---- imageio.hip
    fn = 'fnn_decode_voxels'
    g = (hp(), 4, 0, 64, 0, 1.0, 0.0, hp(4096), NULL)
    R += _nulls(fn, g, (0, 7), INVALID, 'NULL argument')
    R += [(fn + '-negative-n_vox', fn, _with(g, 3, -1), INVALID, 'negative n_vox'),
          (fn + '-raw-misaligned', fn, _with(g, 0, hp(8)), INVALID, fn + ': raw must be 16-byte aligned'),
          (fn + '-out-misaligned', fn, _with(g, 7, hp(4098)), INVALID, fn + ': out must be 4-byte aligned'),
          (fn + '-datatype', fn, _with(g, 1, 128), UNSUPPORTED, fn + NIFTI),
          (fn + '-host', fn, g, INVALID, fn + DEV)]
    fn = 'fnn_decode_labels'
    g = (hp(), 4, 0, 64, 0, 1.0, 0.0, 2, hp(4096), hp(8192), NULL)
    R += _nulls(fn, g, (0, 8, 9), INVALID, 'NULL argument')
    R += [(fn + '-negative-n_vox', fn, _with(g, 3, -1), INVALID, 'negative n_vox'),
          (fn + '-out_bytes', fn, _with(g, 7, 4), INVALID, fn + ': out_bytes must be 1 (uint8) or 2 (uint16)'),
          (fn + '-raw-misaligned', fn, _with(g, 0, hp(4)), INVALID, fn + ': raw must be 16-byte aligned'),
          (fn + '-out-misaligned', fn, _with(g, 8, hp(4097)), INVALID, fn + ': out must be aligned to its element'),
          (fn + '-status-misaligned', fn, _with(g, 9, hp(8194)), INVALID, fn + ': status must be 4-byte aligned'),
          (fn + '-datatype', fn, _with(g, 1, 1536), UNSUPPORTED, fn + NIFTI),
          (fn + '-host', fn, g, INVALID, fn + DEV),
          (fn + '-host-status-empty', fn, _with(g, 3, 0), INVALID, fn + DEV)]
    # ---- reorient.hip
    fn = 'fnn_reorient'
    g = (hp(), 2, S3, ID, i32(0, 0, 0), hp(4096), NULL)
    R += _nulls(fn, g, (0, 2, 3, 4, 5), INVALID, 'NULL argument')
    R += [(f'{fn}-perm-{n}', fn, _with(g, 3, p), INVALID, fn + ': src_axis must be a permutation of 0, 1, 2') for n, p in BAD_PERMS.items()]
    R += [(fn + '-elem_bytes', fn, _with(g, 1, 8), UNSUPPORTED, fn + ': elements of 1, 2 or 4 bytes are served'),
          (fn + '-negative-extent', fn, _with(g, 2, i64(4, -4, 4)), INVALID, fn + ': negative extent'),
          (fn + '-overflow', fn, _with(g, 2, i64(1 << 31, 1 << 31, 1 << 31)), UNSUPPORTED, fn + ': too many elements for one launch'),
          (fn + '-misaligned', fn, _with(g, 5, hp(4097)), INVALID, fn + ': in and out must be aligned to the element size'),
          (fn + '-overlap', fn, _with(g, 5, hp(64)), INVALID, fn + ': in and out overlap'),
          (fn + '-host', fn, g, INVALID, fn + DEV)]
    # ---- deflate.hip
    fn = 'fnn_deflate_labels'
    g = (hp(), 1, 64, 0, hp(4096), 4096, O64, O32, OU32, NULL)
    R += _nulls(fn, g, (0, 4, 6, 7, 8), INVALID, 'NULL argument')
    R += [(fn + '-elem_bytes', fn, _with(g, 1, 4), INVALID, fn + ': labels of 1 or 2 bytes are served'),
          (fn + '-negative-count', fn, _with(g, 2, -1), INVALID, fn + ': negative element count'),
          (fn + '-misaligned', fn, _with(g, 0, hp(8)), INVALID, fn + ': in must be aligned to 16 bytes'),
          (fn + '-too-many', fn, _with(g, 2, 1 << 46), UNSUPPORTED, fn + ': too many bytes for one launch sequence'),
          (fn + '-out_cap', fn, _with(g, 5, 64), INVALID, fn + ': out_cap is below fnn_deflate_bound'),
          (fn + '-host', fn, g, INVALID, fn + DEV)]
    # ---- deflate_masks.hip
    for fn, g, extra_null, devmsg in (
            ('fnn_deflate_masks_count', (hp(), 1, 64, i32(1, 2), 2, hp(4096), 1 << 20, O64, OU32, NULL), (7, 8),
             ' needs device pointers for in and work (no CPU path)'),
            ('fnn_deflate_masks_emit', (hp(), 1, 64, i32(1, 2), 2, hp(4096), hp(8192), 4096, NULL), (6,),
             ' needs device pointers for in, work and out (no CPU path)')):
        R += _nulls(fn, g, (0, 3, 5) + extra_null, INVALID, fn + ': NULL argument')
        R += [(fn + '-elem_bytes', fn, _with(g, 1, 3), INVALID, fn + ': labels of 1 or 2 bytes are served'),
              (fn + '-negative-count', fn, _with(g, 2, -1), INVALID, fn + ': negative element count'),
              (fn + '-in-misaligned', fn, _with(g, 0, hp(8)), INVALID, fn + ': in must be aligned to 16 bytes'),
              (fn + '-work-misaligned', fn, _with(g, 5, hp(4104)), INVALID, fn + ': work must be aligned to 16 bytes'),
              (fn + '-n_labels0', fn, _with(g, 4, 0), INVALID, fn + ': n_labels must be at least 1'),
              (fn + '-label-range', fn, _with(g, 3, i32(1, 65536)), INVALID, fn + ': a label lies outside [0, 65535]'),
              (fn + '-label-twice', fn, _with(g, 3, i32(2, 2)), INVALID, fn + ': a label is named twice (duplicate)'),
              (fn + '-too-many', fn, _with(g, 2, 1 << 46), UNSUPPORTED, fn + ': too many elements for one launch sequence'),
              (fn + '-host', fn, g, INVALID, fn + devmsg)]
    R += [('fnn_deflate_masks_count-work_cap', 'fnn_deflate_masks_count', (hp(), 1, 64, i32(1, 2), 2, hp(4096), 16, O64, OU32, NULL),
           INVALID, 'fnn_deflate_masks_count: work_cap is below fnn_deflate_masks_work_bytes'),
          ('fnn_deflate_masks_emit-negative-out_cap', 'fnn_deflate_masks_emit', (hp(), 1, 64, i32(1, 2), 2, hp(4096), hp(8192), -1, NULL),
           INVALID, 'fnn_deflate_masks_emit: out_cap is negative')]
    return R


ROWS = _rows()
ENTRIES = ['fnn_nonzero_bbox', 'fnn_preprocess', 'fnn_revert_labels', 'fnn_export_probabilities', 'fnn_resample',
           'fnn_resample_torch', 'fnn_resample_torch_seg', 'fnn_resample_labels', 'fnn_keep_largest_components',
           'fnn_ensemble_export', 'fnn_average_probabilities', 'fnn_confusion_counts', 'fnn_decode_voxels', 'fnn_decode_labels',
           'fnn_reorient', 'fnn_deflate_labels', 'fnn_deflate_masks_count', 'fnn_deflate_masks_emit']


def call(row):
    _, fn, args, _, _ = row
    lib = capi.load_library()
    lib.fnn_last_error.restype = C.c_char_p
    code = getattr(lib, fn)(*args)
    return code, lib.fnn_last_error(None).decode()


@pytest.mark.parametrize('row', ROWS, ids=[r[0] for r in ROWS])
def test_refusal_code_and_text(row):
    assert call(row) == (row[3], row[4])


def test_the_table_covers_every_entry_point_and_names_each_row_once():
    assert sorted({r[1] for r in ROWS}) == sorted(ENTRIES)
    assert len({r[0] for r in ROWS}) == len(ROWS)
    for fn in ENTRIES:                                              # each one: a NULL (or missing map) row and a host-memory row
        ids = [r[0] for r in ROWS if r[1] == fn]
        assert any('-null-' in i for i in ids) and any(i.endswith('-host') for i in ids), fn
