"""nnU-Net's evaluation of predictions, on label arrays, counted on the GPU.

Replaces ``nnunetv2.evaluation.evaluate_predictions`` (evaluation/evaluate_predictions.py) without the image
reader-writer: ``compute_metrics`` (:88-118) and the aggregation of ``compute_metrics_on_folder`` (:149-175) take numpy
arrays or torch tensors, and ``save_summary_json`` / ``load_summary_json`` (:33-60) keep the reference's file format.

``compute_metrics_on_folder`` / ``compute_metrics_on_folder2`` / ``compute_metrics_on_folder_simple`` (:121-212) are the
reference's folder commands on top of it: the label files are read as labels on the device (``NiftiIO.read_label_map``'s
kernel), one case at a time behind a reader thread.

Two halves:

* device - ``confusion_counts``: one ``fnn_confusion_counts`` pass (csrc/metrics.hip) turns a reference map and 1..4
  predicted maps into exact [reference class][predicted class] matrices.  The classes are the distinct label values
  named by ``labels_or_regions``, in ascending order (``count_classes``), plus "other" for every remaining value;
* host - ``metrics_from_counts``: every label or region (a tuple is a union of labels) gets TP / FP / FN / TN from the
  matrix, and the per-case dict is built with the reference's numpy scalar types and expressions, so the floats are
  bit-identical to the reference's.  This half needs no GPU.

Beyond the reference, on request (``surface_metrics=True``): the boundary metrics HD, HD95, ASSD and NSD with medpy's
definitions.  ``surface_distances`` gets the exact distances from every surface voxel of one mask to the surface of the
other from ``fnn_surface_count`` / ``fnn_surface_distances`` (csrc/surface.hip); ``surface_metrics_of`` is the host half,
plain numpy expressions on the downloaded distances.

And (``instance_metrics=True``) the lesion-wise metrics per 26-connected component: detection recall / precision / F1 with
the autoPET rule, the voxels of missed and of false-positive lesions, and panoptic quality at IoU > 0.5.
``instance_overlaps`` gets both maps' component sizes and the pairs' overlaps from ``fnn_instance_overlaps``
(csrc/instance.hip); ``instance_metrics_of`` is the host half, numpy expressions on exact integers.
"""
from __future__ import annotations

import copy
import json
import math
import os
from typing import List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import capi

LabelOrRegion = Union[int, Tuple[int, ...]]
MAX_PREDICTIONS_PER_PASS = 4


# ---- classes of the count matrix ------------------------------------------------------------------------------------
def _members(label_or_region) -> List[int]:
    if np.isscalar(label_or_region) or isinstance(label_or_region, (int, np.integer)):
        return [int(label_or_region)]
    return [int(v) for v in label_or_region]


def count_classes(labels_or_regions: Sequence[LabelOrRegion]) -> List[int]:
    """The label values that get a class of their own, ascending; class ``len(result)`` is "other"."""
    vals = sorted({v for r in labels_or_regions for v in _members(r)})
    for v in vals:
        if v < 0 or v > 65535:
            raise ValueError(f'label {v} is outside 0..65535')
    if len(vals) > 255:
        raise ValueError(f'at most 255 distinct labels can be evaluated at once, got {len(vals)}')
    return vals


def class_table(values: Sequence[int]) -> np.ndarray:
    """class_of_value for fnn_confusion_counts: class index of each label value, -1 for "other"."""
    table = np.full(max(values) + 1 if len(values) else 0, -1, np.int32)
    for k, v in enumerate(values):
        table[v] = k
    return table


# ---- host half: metrics from a count matrix -------------------------------------------------------------------------
def tp_fp_fn_tn(counts: np.ndarray, classes: Sequence[int]):
    """(tp, fp, fn, tn) as numpy int64 of the union of ``classes`` (class indices) in one [C+1, C+1] matrix."""
    counts = np.asarray(counts, dtype=np.int64)
    inside = np.zeros(counts.shape[0], bool)
    inside[list(classes)] = True
    tp = counts[inside][:, inside].sum(dtype=np.int64)
    fp = counts[~inside][:, inside].sum(dtype=np.int64)
    fn = counts[inside][:, ~inside].sum(dtype=np.int64)
    tn = counts[~inside][:, ~inside].sum(dtype=np.int64)
    return tp, fp, fn, tn


def metrics_of(tp, fp, fn, tn) -> dict:
    """One entry of compute_metrics' ``results['metrics']`` (evaluate_predictions.py:104-117), same expressions."""
    out = {}
    if tp + fp + fn == 0:
        out['Dice'] = np.nan
        out['IoU'] = np.nan
    else:
        out['Dice'] = 2 * tp / (2 * tp + fp + fn)
        out['IoU'] = tp / (tp + fp + fn)
    out['FP'] = fp
    out['TP'] = tp
    out['FN'] = fn
    out['TN'] = tn
    out['n_pred'] = fp + tp
    out['n_ref'] = fn + tp
    return out


def metrics_from_counts(counts: np.ndarray, labels_or_regions: Sequence[LabelOrRegion]) -> dict:
    """``{label_or_region: {'Dice', 'IoU', 'FP', 'TP', 'FN', 'TN', 'n_pred', 'n_ref'}}`` from one [C+1, C+1] matrix
    whose classes are ``count_classes(labels_or_regions)``."""
    values = count_classes(labels_or_regions)
    counts = np.asarray(counts)
    if counts.shape != (len(values) + 1, len(values) + 1):
        raise ValueError(f'count matrix of shape {counts.shape} does not match {len(values)} classes + other')
    index = {v: k for k, v in enumerate(values)}
    return {r: metrics_of(*tp_fp_fn_tn(counts, [index[v] for v in _members(r)])) for r in labels_or_regions}


def case_result(metrics: dict, reference_file=None, prediction_file=None) -> dict:
    return {'reference_file': reference_file, 'prediction_file': prediction_file, 'metrics': metrics}


def json_ready(obj):
    """A copy with numpy scalars as Python numbers, numpy integer keys as int, 1-D arrays and tuples as lists of
    Python numbers; NaN stays a float.  What compute_metrics_on_folder makes of its results before it returns them."""
    if isinstance(obj, dict):
        return {(int(k) if isinstance(k, np.integer) else k): json_ready(v) for k, v in obj.items()}
    if isinstance(obj, np.ndarray):
        if obj.ndim != 1:
            raise ValueError('only 1-D arrays can be exported')
        return [json_ready(v) for v in obj.tolist()]
    if isinstance(obj, (list, tuple)):
        return type(obj)(json_ready(v) for v in obj)
    if isinstance(obj, np.bool_):
        return bool(obj)
    if isinstance(obj, np.integer):
        return int(obj)
    if isinstance(obj, np.floating):
        return float(obj)
    return obj


def aggregate(results: List[dict], labels_or_regions: Sequence[LabelOrRegion]) -> dict:
    """compute_metrics_on_folder's summary (:149-175) of per-case results: nanmean per class and metric, and
    ``foreground_mean`` as the mean over every class whose key is not 0."""
    if not results:
        raise ValueError('no case to aggregate')
    metric_list = list(results[0]['metrics'][labels_or_regions[0]].keys())
    means = {}
    for r in labels_or_regions:
        means[r] = {}
        for m in metric_list:
            vals = [i['metrics'][r][m] for i in results]
            if all(isinstance(v, float) and math.isnan(v) for v in vals):
                means[r][m] = np.float64(np.nan)     # np.nanmean of all-NaN, without its warning
            else:
                means[r][m] = np.nanmean(vals)
    foreground_mean = {}
    for m in metric_list:
        values = [means[k][m] for k in means.keys() if not (k == 0 or k == '0')]
        foreground_mean[m] = np.mean(values)
    return {'metric_per_case': [json_ready(i) for i in results], 'mean': json_ready(means),
            'foreground_mean': json_ready(foreground_mean)}


# ---- summary.json -----------------------------------------------------------------------------------------------------
def label_or_region_to_key(label_or_region) -> str:
    return str(label_or_region)


def key_to_label_or_region(key: str):
    try:
        return int(key)
    except ValueError:
        parts = key.replace('(', '').replace(')', '').split(',')
        return tuple(int(p) for p in parts if len(p) > 0)


def _dump_json(obj, path: str):
    with open(path, 'w') as f:
        json.dump(json_ready(obj), f, sort_keys=True, indent=4)


def save_summary_json(results: dict, output_file: str):
    """The reference's summary.json: label / region keys as strings, sorted keys, NaN written as NaN."""
    out = copy.deepcopy(results)
    out['mean'] = {label_or_region_to_key(k): v for k, v in results['mean'].items()}
    for case in out['metric_per_case']:
        case['metrics'] = {label_or_region_to_key(k): v for k, v in case['metrics'].items()}
    _dump_json(out, output_file)


def load_summary_json(filename: str) -> dict:
    with open(filename) as f:
        results = json.load(f)
    results['mean'] = {key_to_label_or_region(k): v for k, v in results['mean'].items()}
    for case in results['metric_per_case']:
        case['metrics'] = {key_to_label_or_region(k): v for k, v in case['metrics'].items()}
    return results


# ---- device half -------------------------------------------------------------------------------------------------------
def _device() -> torch.device:
    if not torch.cuda.is_available():
        raise RuntimeError('evaluation counts on an AMD GPU through the HIP engine; no GPU is visible')
    return torch.device('cuda', torch.cuda.current_device())


def check_label_map(seg) -> Tuple[int, int]:
    """(min, max) of an integer label map with values in 0..65535 (numpy or torch); anything else raises ValueError."""
    if isinstance(seg, torch.Tensor):
        if seg.dtype == torch.bool or seg.dtype.is_floating_point or seg.dtype.is_complex:
            raise ValueError(f'label maps must have an integer dtype, got {seg.dtype}')
        if seg.numel() == 0:
            return 0, 0
        lo, hi = int(seg.min()), int(seg.max())
    else:
        arr = np.asarray(seg)
        if arr.dtype.kind not in 'iu':
            raise ValueError(f'label maps must have an integer dtype, got {arr.dtype}')
        if arr.size == 0:
            return 0, 0
        lo, hi = int(arr.min()), int(arr.max())
    if lo < 0 or hi > 65535:
        raise ValueError(f'label values must lie in 0..65535 (got {lo}..{hi})')
    return lo, hi


def _is_u8(seg) -> bool:
    return seg.dtype == torch.uint8 if isinstance(seg, torch.Tensor) else np.asarray(seg).dtype == np.uint8


def to_device_labels(seg, u16: bool, device: torch.device) -> torch.Tensor:
    """A flat, contiguous, 16-byte aligned device tensor the kernel reads: uint8, or uint16 bits in int16.  A device
    uint8 map is used in place when it already is one; the caller's map is never written."""
    if isinstance(seg, torch.Tensor):
        t = seg if seg.device.type == 'cuda' else seg.to(device)
    else:
        arr = np.asarray(seg)
        t = torch.from_numpy(np.ascontiguousarray(arr if arr.dtype == np.uint8 else arr.astype(np.int32))).to(device)
    if u16:
        t = t.to(torch.int32).to(torch.int16) if t.dtype != torch.int16 else t
    elif t.dtype != torch.uint8:
        t = t.to(torch.uint8)
    t = t.reshape(-1)
    if not t.is_contiguous() or t.data_ptr() % 16:
        t = t.clone(memory_format=torch.contiguous_format)
    return t


def _shape(seg) -> tuple:
    return tuple(seg.shape) if isinstance(seg, torch.Tensor) else np.shape(seg)


def confusion_counts(seg_ref, seg_preds: Sequence, values: Sequence[int], ignore_label: Optional[int] = None,
                     checked: bool = False) -> np.ndarray:
    """Exact int64 [len(seg_preds), C + 1, C + 1] matrices [reference class][predicted class] of ``seg_ref`` against
    every map in ``seg_preds``; class k is label value ``values[k]``, class C = len(values) every other value.
    Reference voxels equal to ``ignore_label`` are not counted.  The reference map is read once per 4 predictions."""
    if len(seg_preds) == 0:
        raise ValueError('at least one prediction is needed')
    maps = [seg_ref] + list(seg_preds)
    for s in maps[1:]:
        if _shape(s) != _shape(seg_ref):
            raise ValueError(f'shape mismatch: reference {_shape(seg_ref)}, prediction {_shape(s)}')
    if not checked:
        for s in maps:
            check_label_map(s)
    u16 = not all(_is_u8(s) for s in maps)
    values = list(values)
    table = class_table(values)
    ignore = -1 if ignore_label is None else int(ignore_label)
    dev = next((s.device for s in maps if isinstance(s, torch.Tensor) and s.device.type == 'cuda'), None) or _device()
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        ref = to_device_labels(seg_ref, u16, dev)
        out = []
        for k in range(0, len(seg_preds), MAX_PREDICTIONS_PER_PASS):
            preds = [to_device_labels(p, u16, dev) for p in seg_preds[k:k + MAX_PREDICTIONS_PER_PASS]]
            out.append(capi.confusion_counts(ref.data_ptr(), [p.data_ptr() for p in preds], u16, ref.numel(), table,
                                             len(values), ignore, stream))
    return np.concatenate(out, axis=0)


def _check_ignore(labels_or_regions, ignore_label):
    if ignore_label is not None and any(int(ignore_label) in _members(r) for r in labels_or_regions):
        raise ValueError(f'ignore label {ignore_label} is also one of the evaluated labels')


# ---- surface distances and the boundary metrics ---------------------------------------------------------------------------
SURFACE_KEYS = ('HD', 'HD95', 'ASSD', 'NSD', 'n_surf_pred', 'n_surf_ref')
MAX_SURFACE_REGIONS = 1024


def _check_surface_request(surface_metrics: bool, ignore_label, spacing):
    if not surface_metrics:
        return
    if ignore_label is not None:
        raise ValueError(f'surface metrics are refused together with an ignore label ({ignore_label}): a boundary next to '
                         f'ignored voxels has no agreed meaning')
    if spacing is None:
        raise ValueError('surface metrics need the voxel spacing (z, y, x)')


def region_members(labels_or_regions: Sequence[LabelOrRegion]) -> np.ndarray:
    """member for fnn_surface_count: uint8 [n_regions, largest label + 1], 1 where the label belongs to the region."""
    regions = [_members(r) for r in labels_or_regions]
    if not 1 <= len(regions) <= MAX_SURFACE_REGIONS:
        raise ValueError(f'1..{MAX_SURFACE_REGIONS} labels or regions can be measured at once, got {len(regions)}')
    for v in (v for r in regions for v in r):
        if v < 0 or v > 65535:
            raise ValueError(f'label {v} is outside 0..65535')
    member = np.zeros((len(regions), max((v for r in regions for v in r), default=0) + 1), np.uint8)
    for k, r in enumerate(regions):
        member[k, r] = 1
    return member


def _volume_shape(shape: tuple) -> tuple:
    """(z, y, x) of a label map's shape; leading axes of length 1 (the reference's [1, X, Y, Z]) are dropped."""
    shape = tuple(int(i) for i in shape)
    while len(shape) > 3 and shape[0] == 1:
        shape = shape[1:]
    if len(shape) != 3:
        raise ValueError(f'surface distances are measured on 3-D label maps, got shape {shape}')
    return shape


def _spacing3(spacing) -> tuple:
    sp = tuple(float(s) for s in np.asarray(spacing, dtype=np.float64).reshape(-1))
    if len(sp) != 3 or not all(math.isfinite(s) and s > 0 for s in sp):
        raise ValueError(f'spacing must be three finite positive numbers (z, y, x), got {spacing}')
    return sp


def _surface_distances(seg_ref, seg_pred, labels_or_regions, spacing, checked: bool = False):
    """-> ({r: (dp, dr)}, n_surface int64 [n_regions, 2] = |S(ref_r)|, |S(pred_r)|, boxes int64 [n_regions, 6])."""
    labels_or_regions = list(labels_or_regions)
    if _shape(seg_ref) != _shape(seg_pred):
        raise ValueError(f'shape mismatch: reference {_shape(seg_ref)}, prediction {_shape(seg_pred)}')
    shape, sp, member = _volume_shape(_shape(seg_ref)), _spacing3(spacing), region_members(labels_or_regions)
    if not checked:
        for s in (seg_ref, seg_pred):
            check_label_map(s)
    u16 = not (_is_u8(seg_ref) and _is_u8(seg_pred))
    dev = next((s.device for s in (seg_ref, seg_pred) if isinstance(s, torch.Tensor) and s.device.type == 'cuda'), None) or _device()
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        ref, pred = to_device_labels(seg_ref, u16, dev), to_device_labels(seg_pred, u16, dev)
        n_surface, boxes = capi.surface_count(ref.data_ptr(), pred.data_ptr(), u16, shape, member, stream)
        both = (n_surface[:, 0] > 0) & (n_surface[:, 1] > 0)
        total = int(n_surface[both].sum())
        buf = torch.empty(max(total, 1), dtype=torch.float64, device=dev)
        capi.surface_distances(ref.data_ptr(), pred.data_ptr(), u16, shape, member, sp, buf.data_ptr(), total, stream)
        dist = np.sqrt(buf[:total].cpu().numpy())
    out, at = {}, 0
    for k, r in enumerate(labels_or_regions):
        n_r, n_p = (int(n_surface[k, 0]), int(n_surface[k, 1])) if both[k] else (0, 0)
        out[r] = (dist[at:at + n_p], dist[at + n_p:at + n_p + n_r])
        at += n_p + n_r
    return out, n_surface, boxes


def surface_distances(seg_ref, seg_pred, labels_or_regions: Sequence[LabelOrRegion], spacing) -> dict:
    """``{label_or_region: (dp, dr)}``: float64 arrays of the distances from every surface voxel of the prediction to the
    reference's surface and the other way round, in raster order; both empty where either mask is.  The surface of a mask is
    the mask minus its 6-neighbourhood erosion (outside the volume is background); distances are Euclidean in the units of
    ``spacing`` (z, y, x), bit for bit ``distance_transform_edt(~S(other), sampling=spacing)[S(this)]``.  Label maps as
    ``confusion_counts`` takes them, 3-D (leading axes of length 1 are dropped)."""
    return _surface_distances(seg_ref, seg_pred, labels_or_regions, spacing)[0]


def surface_metrics_of(dp, dr, n_p, n_r, tolerance) -> dict:
    """The host half: medpy's hd / hd95 / assd and the normalised surface Dice at ``tolerance`` from the directed distances
    ``dp`` (prediction to reference) and ``dr``; ``n_p`` / ``n_r`` are the surface voxels of the prediction / reference.
    NaN where either mask is empty (as Dice of an empty pair; medpy raises there)."""
    out = {}
    if n_p == 0 or n_r == 0:
        out['HD'] = out['HD95'] = out['ASSD'] = out['NSD'] = np.nan
    else:
        out['HD'] = max(dp.max(), dr.max())
        out['HD95'] = np.percentile(np.hstack((dp, dr)), 95)
        out['ASSD'] = np.mean((dp.mean(), dr.mean()))
        out['NSD'] = ((dp <= tolerance).sum() + (dr <= tolerance).sum()) / (n_p + n_r)
    out['n_surf_pred'] = np.int64(n_p)
    out['n_surf_ref'] = np.int64(n_r)
    return out


def _tolerance_of(nsd_tolerance, label_or_region) -> float:
    if isinstance(nsd_tolerance, dict):
        if label_or_region not in nsd_tolerance:
            raise ValueError(f'nsd_tolerance names no tolerance for {label_or_region}')
        return float(nsd_tolerance[label_or_region])
    return float(nsd_tolerance)


def compute_surface_metrics(seg_ref, seg_pred, labels_or_regions: Sequence[LabelOrRegion], spacing, nsd_tolerance=1.0,
                            checked: bool = False) -> dict:
    """``{label_or_region: {'HD', 'HD95', 'ASSD', 'NSD', 'n_surf_pred', 'n_surf_ref'}}``.  ``nsd_tolerance``: a number, or a
    dict with one per label or region, in the units of ``spacing``."""
    labels_or_regions = list(labels_or_regions)
    tol = {r: _tolerance_of(nsd_tolerance, r) for r in labels_or_regions}
    dist, n_surface, _ = _surface_distances(seg_ref, seg_pred, labels_or_regions, spacing, checked)
    return {r: surface_metrics_of(*dist[r], int(n_surface[k, 1]), int(n_surface[k, 0]), tol[r])
            for k, r in enumerate(labels_or_regions)}


def _with_keys(metrics: dict, more: dict) -> dict:
    for r, m in metrics.items():
        m.update(more[r])
    return metrics


_with_surface = _with_keys         # its name while the surface keys were the only ones


# ---- connected components, their overlaps and the lesion-wise metrics ----------------------------------------------------
INSTANCE_KEYS = ('n_inst_ref', 'n_inst_pred', 'inst_TP', 'inst_FN', 'inst_FP', 'inst_recall', 'inst_precision', 'inst_F1',
                 'FN_inst_vox', 'FP_inst_vox', 'PQ', 'SQ', 'RQ')
MAX_INSTANCE_GROUPS = 1024


def _check_instance_request(instance_metrics: bool, ignore_label):
    if instance_metrics and ignore_label is not None:
        raise ValueError(f'instance metrics are refused together with an ignore label ({ignore_label}): a component next to '
                         f'ignored voxels has no agreed extent')


def plan_instance_calls(labels_or_regions: Sequence[LabelOrRegion]) -> List[List[int]]:
    """The labels or regions (by position) grouped into calls of pairwise disjoint label sets, by the greedy rule of
    ``postprocessing.plan_passes``: each joins the first call none of whose sets it meets, else opens a new one.  The order
    of the calls means nothing here, so any earlier call may take it, not only the open one; a call holds at most
    ``MAX_INSTANCE_GROUPS`` sets."""
    calls: List[Tuple[List[int], set]] = []
    for k, r in enumerate(labels_or_regions):
        s = set(_members(r))
        for v in s:
            if v < 0 or v > 65535:
                raise ValueError(f'label {v} is outside 0..65535')
        for idx, used in calls:
            if len(idx) < MAX_INSTANCE_GROUPS and not (used & s):
                idx.append(k)
                used |= s
                break
        else:
            calls.append(([k], set(s)))
    return [idx for idx, _ in calls]


def _rank_in_group(group: np.ndarray, n_groups: int) -> np.ndarray:
    """The position of every record among the records of its own group, the order kept."""
    order = np.argsort(group, kind='stable')
    starts = np.searchsorted(group[order], np.arange(n_groups))
    rank = np.empty(len(group), np.int64)
    rank[order] = np.arange(len(group)) - starts[group[order]]
    return rank


def overlaps_from_records(n_out, records: np.ndarray, n_groups: int) -> List[dict]:
    """fnn_instance_overlaps' records -> per group ``{'ref_sizes', 'pred_sizes', 'pairs'}``: the pieces of one (pred component,
    ref component) pair are added up, and roots become positions in the group's size lists.  No GPU call."""
    n_ref, n_pred, n_pieces = (int(v) for v in n_out)
    rec = np.asarray(records, dtype=np.int64).reshape(-1, 3)
    if len(rec) != n_ref + n_pred + n_pieces:
        raise ValueError(f'{len(rec)} records for {n_ref} + {n_pred} + {n_pieces}')
    ref, pred, pieces = rec[:n_ref], rec[n_ref:n_ref + n_pred], rec[n_ref + n_pred:]
    ref_rank, pred_rank = _rank_in_group(ref[:, 0], n_groups), _rank_in_group(pred[:, 0], n_groups)
    at_pred, at_ref = np.searchsorted(pred[:, 1], pieces[:, 0]), np.searchsorted(ref[:, 1], pieces[:, 1])
    piece_group = pred[at_pred, 0] if n_pieces else np.zeros(0, np.int64)
    out = []
    for g in range(n_groups):
        mine = piece_group == g
        pi, ri, size = pred_rank[at_pred[mine]], ref_rank[at_ref[mine]], pieces[mine, 2]
        n_r = int((ref[:, 0] == g).sum())
        uniq, inverse = np.unique(pi * max(n_r, 1) + ri, return_inverse=True)
        overlap = np.zeros(len(uniq), np.int64)
        np.add.at(overlap, inverse.reshape(-1), size)
        pairs = np.stack([uniq // max(n_r, 1), uniq % max(n_r, 1), overlap], axis=1).astype(np.int64).reshape(-1, 3)
        out.append({'ref_sizes': ref[ref[:, 0] == g, 2].copy(), 'pred_sizes': pred[pred[:, 0] == g, 2].copy(), 'pairs': pairs})
    return out


def instance_overlaps(seg_ref, seg_pred, labels_or_regions: Sequence[LabelOrRegion], checked: bool = False, *,
                      first_capacity: Optional[int] = None, calls_made: Optional[list] = None) -> dict:
    """``{label_or_region: {'ref_sizes', 'pred_sizes', 'pairs'}}``: the sizes (int64) of the 26-connected components of the
    reference's and of the prediction's mask, in raster order of the components' first voxels, and ``pairs`` int64 [k, 3] of
    (pred index, ref index, voxels in both) for every pair that shares a voxel, sorted by those indices.  A region is the
    union of its labels; outside the volume is background.  Label maps as ``confusion_counts`` takes them, 3-D (leading axes of
    length 1 are dropped).  Disjoint labels or regions go through one ``fnn_instance_overlaps`` call, overlapping ones
    through ``plan_instance_calls``' few.  ``first_capacity``: ``capi.instance_overlaps``'; ``calls_made`` (a list) receives
    the C calls made per call of the plan."""
    labels_or_regions = list(labels_or_regions)
    if _shape(seg_ref) != _shape(seg_pred):
        raise ValueError(f'shape mismatch: reference {_shape(seg_ref)}, prediction {_shape(seg_pred)}')
    shape, plan = _volume_shape(_shape(seg_ref)), plan_instance_calls(labels_or_regions)
    if not checked:
        for s in (seg_ref, seg_pred):
            check_label_map(s)
    u16 = not (_is_u8(seg_ref) and _is_u8(seg_pred))
    kw = {} if first_capacity is None else {'first_capacity': first_capacity}
    dev = next((s.device for s in (seg_ref, seg_pred) if isinstance(s, torch.Tensor) and s.device.type == 'cuda'), None) or _device()
    out = {}
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        ref, pred = to_device_labels(seg_ref, u16, dev), to_device_labels(seg_pred, u16, dev)
        for idx in plan:
            sets = [_members(labels_or_regions[k]) for k in idx]
            table = np.full(max((v for s in sets for v in s), default=-1) + 1, -1, np.int32)
            for g, s in enumerate(sets):
                table[s] = g
            n_out, records, calls = capi.instance_overlaps(ref.data_ptr(), pred.data_ptr(), u16, shape, table, len(idx), stream, **kw)
            if calls_made is not None:
                calls_made.append(calls)
            for k, lists in zip(idx, overlaps_from_records(n_out, records, len(idx))):
                out[labels_or_regions[k]] = lists
    return {r: out[r] for r in labels_or_regions}


def instance_metrics_of(ref_sizes, pred_sizes, pairs) -> dict:
    """The host half: ``INSTANCE_KEYS`` from the component sizes of the reference (n of them) and of the prediction (m) and
    the pair table ``(pred index, ref index, overlap)``.  A reference component is detected when anything overlaps it (the
    autoPET rule); a predicted component that touches nothing is a false positive; ``FN_inst_vox`` / ``FP_inst_vox`` are the
    voxels of the undetected / the false-positive components.  Panoptic quality counts the pairs with IoU > 0.5 (at most one
    per component): ``RQ = tp / (tp + (m - tp) / 2 + (n - tp) / 2)``, ``SQ`` their mean IoU in the order of ``pairs`` (0.0
    without one), ``PQ = SQ * RQ``.  Counts are np.int64, ratios np.float64; NaN where a denominator's side is empty.
    Exact integers in, numpy expressions - no GPU call."""
    ref_sizes = np.asarray(ref_sizes, dtype=np.int64).reshape(-1)
    pred_sizes = np.asarray(pred_sizes, dtype=np.int64).reshape(-1)
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 3)
    n, m = np.int64(len(ref_sizes)), np.int64(len(pred_sizes))
    pairs = pairs[pairs[:, 2] > 0]
    hit_ref, hit_pred = np.zeros(n, bool), np.zeros(m, bool)
    hit_pred[pairs[:, 0]] = True
    hit_ref[pairs[:, 1]] = True
    nan = np.float64(np.nan)
    out = {'n_inst_ref': n, 'n_inst_pred': m}
    tp = out['inst_TP'] = hit_ref.sum(dtype=np.int64)
    out['inst_FN'] = n - tp
    fp = out['inst_FP'] = (~hit_pred).sum(dtype=np.int64)
    recall = out['inst_recall'] = tp / n if n > 0 else nan
    precision = out['inst_precision'] = (m - fp) / m if m > 0 else nan
    if np.isnan(recall) or np.isnan(precision):
        out['inst_F1'] = nan
    elif precision + recall == 0:
        out['inst_F1'] = np.float64(0.0)
    else:
        out['inst_F1'] = 2 * precision * recall / (precision + recall)
    out['FN_inst_vox'] = ref_sizes[~hit_ref].sum(dtype=np.int64)
    out['FP_inst_vox'] = pred_sizes[~hit_pred].sum(dtype=np.int64)
    if n == 0 and m == 0:
        out['PQ'] = out['SQ'] = out['RQ'] = nan
        return out
    union = pred_sizes[pairs[:, 0]] + ref_sizes[pairs[:, 1]] - pairs[:, 2]
    matched = 2 * pairs[:, 2] > union                                   # IoU > 0.5 on the integers
    q = matched.sum(dtype=np.int64)
    rq = q / (q + 0.5 * (m - q) + 0.5 * (n - q))
    sq = np.mean(pairs[matched, 2] / union[matched]) if q > 0 else np.float64(0.0)
    out['PQ'] = sq * rq
    out['SQ'] = sq
    out['RQ'] = rq
    return out


def compute_instance_metrics(seg_ref, seg_pred, labels_or_regions: Sequence[LabelOrRegion], checked: bool = False) -> dict:
    """``{label_or_region: {INSTANCE_KEYS}}`` of one case: ``instance_overlaps`` on the device, ``instance_metrics_of`` here."""
    lists = instance_overlaps(seg_ref, seg_pred, labels_or_regions, checked)
    return {r: instance_metrics_of(v['ref_sizes'], v['pred_sizes'], v['pairs']) for r, v in lists.items()}


def compute_metrics(seg_ref, seg_pred, labels_or_regions: Sequence[LabelOrRegion], ignore_label: Optional[int] = None,
                    reference_file=None, prediction_file=None, *, surface_metrics: bool = False, spacing=None,
                    nsd_tolerance=1.0, instance_metrics: bool = False) -> dict:
    """compute_metrics (evaluate_predictions.py:88-118) with arrays in place of the files: numpy arrays or torch
    tensors of one shape (the reference's [1, X, Y, Z] included), integer labels 0..65535.  ``surface_metrics``: every
    label's dict also gets ``compute_surface_metrics``' six keys for ``spacing`` (z, y, x) and ``nsd_tolerance``.
    ``instance_metrics``: and, behind them, ``compute_instance_metrics``' ``INSTANCE_KEYS``."""
    labels_or_regions = list(labels_or_regions)
    _check_ignore(labels_or_regions, ignore_label)
    _check_surface_request(surface_metrics, ignore_label, spacing)
    _check_instance_request(instance_metrics, ignore_label)
    counts = confusion_counts(seg_ref, [seg_pred], count_classes(labels_or_regions), ignore_label)[0]
    metrics = metrics_from_counts(counts, labels_or_regions)
    if surface_metrics:
        _with_keys(metrics, compute_surface_metrics(seg_ref, seg_pred, labels_or_regions, spacing, nsd_tolerance, checked=True))
    if instance_metrics:
        _with_keys(metrics, compute_instance_metrics(seg_ref, seg_pred, labels_or_regions, checked=True))
    return case_result(metrics, reference_file, prediction_file)


def compute_metrics_on_arrays(refs: Sequence, preds: Sequence, labels_or_regions: Sequence[LabelOrRegion],
                              ignore_label: Optional[int] = None, names: Optional[Sequence[str]] = None,
                              output_file: Optional[str] = None, *, surface_metrics: bool = False, spacing=None,
                              nsd_tolerance=1.0, instance_metrics: bool = False) -> dict:
    """compute_metrics_on_folder (evaluate_predictions.py:121-177) on pairs of arrays: ``preds[i]`` is evaluated
    against ``refs[i]``; ``names[i]`` (optional) fills reference_file / prediction_file.  Returns
    ``{'metric_per_case', 'mean', 'foreground_mean'}``; writes it to ``output_file`` (.json) when given.
    ``surface_metrics``, ``instance_metrics``: as ``compute_metrics``; ``spacing`` is one (z, y, x) for all cases or one per
    case."""
    if output_file is not None and not output_file.endswith('.json'):
        raise ValueError('output_file should end with .json')
    if len(refs) != len(preds):
        raise ValueError(f'{len(refs)} references for {len(preds)} predictions')
    if names is not None and len(names) != len(preds):
        raise ValueError('one name per case expected')
    labels_or_regions = list(labels_or_regions)
    _check_surface_request(surface_metrics, ignore_label, spacing)
    _check_instance_request(instance_metrics, ignore_label)
    spacings = [None] * len(preds)
    if surface_metrics:
        spacings = [spacing] * len(preds) if np.ndim(spacing) == 1 else list(spacing)
        if len(spacings) != len(preds):
            raise ValueError('one spacing for all cases or one per case expected')
    results = [compute_metrics(r, p, labels_or_regions, ignore_label,
                               None if names is None else names[i], None if names is None else names[i],
                               surface_metrics=surface_metrics, spacing=spacings[i], nsd_tolerance=nsd_tolerance,
                               instance_metrics=instance_metrics)
               for i, (r, p) in enumerate(zip(refs, preds))]
    summary = aggregate(results, labels_or_regions)
    if output_file is not None:
        save_summary_json(summary, output_file)
    return summary


# ---- folders -----------------------------------------------------------------------------------------------------------
DEFAULT_NUM_PROCESSES = 8


def _paired_files(folder_ref: str, folder_pred: str, file_ending: str, chill: bool):
    """The reference's pairing (:133-139): the cases are the sorted prediction files, the reference list is built from
    their names; ``chill=False`` asserts that every reference file has a prediction."""
    from .label_folders import subfiles
    files_pred = subfiles(folder_pred, suffix=file_ending, join=False)
    files_ref = subfiles(folder_ref, suffix=file_ending, join=False)
    if not chill:
        present = [os.path.isfile(os.path.join(folder_pred, i)) for i in files_ref]
        assert all(present), 'Not all files in folder_ref exist in folder_pred'
    return [os.path.join(folder_ref, i) for i in files_pred], [os.path.join(folder_pred, i) for i in files_pred]


def compute_metrics_on_files(files_ref: Sequence[str], files_pred: Sequence[str], image_reader_writer,
                             labels_or_regions: Sequence[LabelOrRegion], ignore_label: Optional[int] = None, *,
                             surface_metrics: bool = False, spacing=None, nsd_tolerance=1.0,
                             instance_metrics: bool = False) -> List[dict]:
    """``compute_metrics`` (:88-118) for every pair of label files: both are decoded to labels on the device and counted
    by ``fnn_confusion_counts``; the reader thread inflates the next pair meanwhile.  A pair of different shapes raises a
    ValueError that names both files.  ``surface_metrics``: every label's dict also gets ``compute_surface_metrics``' six
    keys, measured with the spacing of the reference file; a prediction whose spacing differs (``np.allclose``) raises a
    ValueError that names both files.  ``spacing`` (z, y, x), when given, is used for every case in place of the files' own,
    which are then not compared.  ``instance_metrics``: and, behind them, ``compute_instance_metrics``' ``INSTANCE_KEYS``, from the
    two maps already on the device."""
    from .label_folders import run_label_cases
    labels_or_regions = list(labels_or_regions)
    _check_ignore(labels_or_regions, ignore_label)
    _check_surface_request(surface_metrics, ignore_label, ())
    _check_instance_request(instance_metrics, ignore_label)
    values = count_classes(labels_or_regions)
    cases = [[r, p] for r, p in zip(files_ref, files_pred)]

    def run(i, maps):
        (ref, ref_props), (pred, pred_props) = maps
        if tuple(ref.shape) != tuple(pred.shape):
            raise ValueError(f'shape mismatch: reference {cases[i][0]} is {tuple(ref.shape)}, prediction {cases[i][1]} is '
                             f'{tuple(pred.shape)}')
        counts = confusion_counts(ref, [pred], values, ignore_label, checked=True)[0]
        metrics = metrics_from_counts(counts, labels_or_regions)
        if surface_metrics:
            of_ref, of_pred = list(ref_props['spacing']), list(pred_props['spacing'])
            if spacing is None and (len(of_ref) != len(of_pred) or not np.allclose(of_ref, of_pred)):
                raise ValueError(f'spacing mismatch: reference {cases[i][0]} has {tuple(of_ref)}, prediction {cases[i][1]} has '
                                 f'{tuple(of_pred)}')
            _with_keys(metrics, compute_surface_metrics(ref, pred, labels_or_regions, of_ref if spacing is None else spacing,
                                                        nsd_tolerance, checked=True))
        if instance_metrics:
            _with_keys(metrics, compute_instance_metrics(ref, pred, labels_or_regions, checked=True))
        return case_result(metrics, cases[i][0], cases[i][1]), None

    return run_label_cases(image_reader_writer, cases, run)


def compute_metrics_on_folder(folder_ref: str, folder_pred: str, output_file: Optional[str], image_reader_writer,
                              file_ending: str, regions_or_labels: Sequence[LabelOrRegion], ignore_label: Optional[int] = None,
                              num_processes: int = DEFAULT_NUM_PROCESSES, chill: bool = True, *, surface_metrics: bool = False,
                              spacing=None, nsd_tolerance=1.0, instance_metrics: bool = False) -> dict:
    """compute_metrics_on_folder (:121-173).  ``output_file`` must end with .json; can be None.  ``image_reader_writer``: an
    instance of this package's reader-writer classes.  ``num_processes`` is accepted and ignored: no process is started.
    ``surface_metrics`` / ``spacing`` / ``nsd_tolerance`` / ``instance_metrics``: as ``compute_metrics_on_files``."""
    if output_file is not None:
        assert output_file.endswith('.json'), 'output_file should end with .json'
    files_ref, files_pred = _paired_files(folder_ref, folder_pred, file_ending, chill)
    regions_or_labels = list(regions_or_labels)
    results = compute_metrics_on_files(files_ref, files_pred, image_reader_writer, regions_or_labels, ignore_label,
                                       surface_metrics=surface_metrics, spacing=spacing, nsd_tolerance=nsd_tolerance,
                                       instance_metrics=instance_metrics)
    result = aggregate(results, regions_or_labels)
    if output_file is not None:
        save_summary_json(result, output_file)
    return result


def compute_metrics_on_folder2(folder_ref: str, folder_pred: str, dataset_json_file: str, plans_file: str,
                               output_file: Optional[str] = None, num_processes: int = DEFAULT_NUM_PROCESSES,
                               chill: bool = False, inflate_on_device=False, *, surface_metrics: bool = False,
                               spacing=None, nsd_tolerance=1.0, instance_metrics: bool = False):
    """compute_metrics_on_folder2 (:177-196): labels or regions, ignore label, file ending and the reader-writer from
    ``dataset.json`` and the plans; ``output_file`` defaults to ``<folder_pred>/summary.json``.  ``inflate_on_device``: label
    files written with ``compress_on_device=True`` are inflated on the GPU (``NiftiIO(inflate_on_device=True)``);
    ``inflate_on_device='dynamic'`` serves files written with ``compress_on_device='dynamic'`` too.
    ``surface_metrics`` / ``spacing`` / ``nsd_tolerance`` / ``instance_metrics``: as ``compute_metrics_on_files``."""
    from .imageio import determine_reader_writer_from_dataset_json
    from .label_folders import load_json
    from .plans import PlansManager
    dataset_json = load_json(dataset_json_file)
    rw = determine_reader_writer_from_dataset_json(dataset_json)(inflate_on_device=inflate_on_device)
    if output_file is None:
        output_file = os.path.join(folder_pred, 'summary.json')
    lm = PlansManager(plans_file).get_label_manager(dataset_json)
    compute_metrics_on_folder(folder_ref, folder_pred, output_file, rw, dataset_json['file_ending'],
                              lm.foreground_regions if lm.has_regions else lm.foreground_labels, lm.ignore_label,
                              num_processes, chill=chill, surface_metrics=surface_metrics, spacing=spacing,
                              nsd_tolerance=nsd_tolerance, instance_metrics=instance_metrics)


def compute_metrics_on_folder_simple(folder_ref: str, folder_pred: str, labels: Sequence[int], output_file: Optional[str] = None,
                                     num_processes: int = DEFAULT_NUM_PROCESSES, ignore_label: Optional[int] = None,
                                     chill: bool = False, inflate_on_device=False, *, surface_metrics: bool = False,
                                     spacing=None, nsd_tolerance=1.0, instance_metrics: bool = False):
    """compute_metrics_on_folder_simple (:199-212): the file ending is that of the first reference file (``.nii.gz``
    whole, where the reference's ``os.path.splitext`` would keep ``.gz`` and then match the same files).
    ``inflate_on_device``, ``surface_metrics``, ``spacing``, ``nsd_tolerance``, ``instance_metrics``: as
    ``compute_metrics_on_folder2``."""
    from .imageio import determine_reader_writer_from_file_ending
    from .label_folders import subfiles
    example_file = subfiles(folder_ref, join=True)[0]
    file_ending = '.nii.gz' if example_file.lower().endswith('.nii.gz') else os.path.splitext(example_file)[-1]
    rw = determine_reader_writer_from_file_ending(file_ending)(inflate_on_device=inflate_on_device)
    if output_file is None:
        output_file = os.path.join(folder_pred, 'summary.json')
    compute_metrics_on_folder(folder_ref, folder_pred, output_file, rw, file_ending, labels, ignore_label=ignore_label,
                              num_processes=num_processes, chill=chill, surface_metrics=surface_metrics, spacing=spacing,
                              nsd_tolerance=nsd_tolerance, instance_metrics=instance_metrics)
