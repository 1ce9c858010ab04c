"""nnU-Net's connected-component postprocessing on the GPU.

Replaces ``nnunetv2.postprocessing.remove_connected_components`` (postprocessing/remove_connected_components.py):
``remove_all_but_largest_component_from_segmentation`` (:21-33), ``apply_postprocessing`` (:36-39) and the
``postprocessing.pkl`` that ``determine_postprocessing`` writes (:221, ``save_pickle((pp_fns, pp_fn_kwargs))``).

The rule implemented (acvl_utils ``remove_all_but_largest_component`` as the reference calls it):

* the mask of a step is ``seg in S``, S the union of ``labels_or_regions`` - an int is one label, a tuple a region
  (evaluation/evaluate_predictions.py:66-73), a non-list argument one member;
* the mask is labelled with full connectivity (skimage ``label(connectivity=None)``): 26 neighbours in 3-D, 8 in 2-D;
* every component whose size equals the largest is kept (ties keep all of them); an empty mask changes nothing;
* voxels in the mask and not kept become ``background_label``; the input is not modified, dtype and shape are kept.

The labelling is ``fnn_keep_largest_components`` (csrc/postprocess.hip), which handles several disjoint label sets in
one pass.  ``load_postprocess_save`` (:42-50) and ``apply_postprocessing_to_folder`` (:247-294) do the same for label files:
read as labels on the device, post-processed there and written by the predictions' writer behind a reader and a writer
thread; ``determine_postprocessing_on_folder`` is the reference's search on folders (postprocessing_search.py).
``apply_postprocessing`` fuses consecutive steps into one pass where that gives the sequential result
(``plan_passes``).  There is no CPU path for this module's own steps.

Two more steps run on the device, the "small region filtering and hole filling" the reference's inference front end names
without shipping their source; both are defined by scipy's published behaviour:

* ``remove_small_components_from_segmentation`` (``fnn_remove_small_components``): the mask ``seg in S`` is labelled like
  ``ndimage.label`` with ``generate_binary_structure(ndim, ndim)`` (``connectivity=26``) or ``(ndim, 1)`` (``6``); every
  component with fewer voxels than ``min_size`` becomes ``background_label``, one of exactly ``min_size`` is kept;
* ``fill_holes_in_segmentation`` (``fnn_fill_holes``): ``holes = ndimage.binary_fill_holes(seg in S) & ~(seg in S)``, default
  (cross) structure, on the 2-D array for a 2-D map; hole voxels whose value is ``background_label`` become ``fill_label``,
  another label that lies inside a hole stays.

The "morphological operations" of that list run on the device too (``fnn_binary_morphology``, csrc/morph.hip):
``binary_dilation_in_segmentation``, ``binary_erosion_in_segmentation``, ``binary_opening_in_segmentation`` and
``binary_closing_in_segmentation``.  With ``M = seg in S``, R is scipy's ``binary_dilation`` / ``binary_erosion`` /
``binary_opening`` / ``binary_closing`` of M with ``structure=generate_binary_structure(ndim, rank)``, ``iterations`` (1..1024;
scipy's "below 1: until nothing changes" is refused) and ``border_value`` (0 or 1), everything else at its default;
``connectivity`` 6, 18 or 26 is rank 1, 2 or 3 (on a 2-D map 18 and 26 both give the full 3x3, 6 the cross; 6 is scipy's
default structure).  The label rule:

* dilation and closing only add: voxels of ``R & ~M`` whose value is ``background_label`` become ``fill_label`` (by default
  the label of S when it has exactly one, as for the holes), any other label there stays, and no voxel of M changes - with
  ``border_value=0`` scipy's closing is not extensive at the border of the map, and what it would take away stays;
* erosion and opening only remove: voxels of ``M & ~R`` become ``background_label`` and no voxel outside M changes - with
  ``border_value=1`` scipy's opening is not anti-extensive, and what it would add is not added.
"""
from __future__ import annotations

import functools
import io
import os
import pickle
from typing import Callable, List, NamedTuple, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import capi
from .case_pipeline import as_plain_labels, compress_mode, labels_for_writer

REFERENCE_NAME = ('nnunetv2.postprocessing.remove_connected_components',
                  'remove_all_but_largest_component_from_segmentation')


def label_set(labels_or_regions) -> frozenset:
    """The label set S of one step: the union of its members (remove_connected_components.py:25-29)."""
    members = labels_or_regions if isinstance(labels_or_regions, list) else [labels_or_regions]
    out = set()
    for m in members:
        if np.isscalar(m) or isinstance(m, (np.integer, int)):
            out.add(int(m))
        else:
            out.update(int(v) for v in m)
    return frozenset(out)


def _is_ours(fn) -> bool:
    if fn is remove_all_but_largest_component_from_segmentation:
        return True
    return (getattr(fn, '__module__', None), getattr(fn, '__qualname__', None)) == REFERENCE_NAME


def _integer(value, name: str) -> int:
    """``value`` as a Python int, or a ValueError naming the argument (bools and non-integral numbers are refused)."""
    if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, float, np.integer, np.floating)) or value != int(value):
        raise ValueError(f'{name} must be an integer, got {value!r}')
    return int(value)


def _small_component_sets(kw: dict) -> Tuple[List[frozenset], List[int], int]:
    """The sets, their ``min_size`` and the connectivity of one ``remove_small_components_from_segmentation`` step, checked."""
    lor, per_member = kw['labels_or_regions'], bool(kw.get('per_member', False))
    conn = kw.get('connectivity', 26)
    if isinstance(conn, (bool, np.bool_)) or conn not in (6, 26):
        raise ValueError(f'connectivity must be 6 or 26, got {conn!r}')
    sets = [label_set(m) for m in lor] if per_member and isinstance(lor, list) else [label_set(lor)]
    for a in range(len(sets)):
        for b in range(a):
            if sets[a] & sets[b]:
                raise ValueError(f'labels_or_regions: with per_member=True the members must be disjoint, '
                                 f'{sorted(sets[a] & sets[b])} are in two of them')
    min_size = kw['min_size']
    if isinstance(min_size, (list, tuple, np.ndarray)):
        if len(min_size) != len(sets):
            raise ValueError(f'min_size has {len(min_size)} entries for {len(sets)} set(s)')
        sizes = [_integer(v, 'min_size') for v in min_size]
    else:
        sizes = [_integer(min_size, 'min_size')] * len(sets)
    if any(v < 0 for v in sizes):
        raise ValueError(f'min_size must not be negative, got {min(sizes)}')
    return sets, sizes, int(conn)


def _hole_set(kw: dict) -> Tuple[frozenset, int, int]:
    """The set, the background and the fill label of one ``fill_holes_in_segmentation`` step, checked."""
    s = label_set(kw['labels_or_regions'])
    bg = _integer(kw.get('background_label', 0), 'background_label')
    fill = kw.get('fill_label')
    if fill is None:
        if len(s) != 1:
            raise ValueError(f'fill_label is required when the set has {len(s)} labels: which of them fills the holes?')
        fill = next(iter(s))
    fill = _integer(fill, 'fill_label')
    if fill == bg:
        raise ValueError(f'fill_label equals background_label ({bg}): nothing would change')
    return s, bg, fill


class MorphParams(NamedTuple):
    """What a morphology step asks of ``fnn_binary_morphology`` beyond its set and background."""
    op: int                                     # capi.FNN_MORPH_DILATE / ERODE / OPEN / CLOSE
    connectivity: int                           # 6, 18 or 26
    iterations: int                             # 1..1024
    border_value: int                           # 0 or 1
    fill_label: int                             # the adding ops'; 0 and unused for erosion and opening


_MORPH_ADDS = (capi.FNN_MORPH_DILATE, capi.FNN_MORPH_CLOSE)


def _morph_step(op: int, kw: dict) -> Tuple[frozenset, int, MorphParams]:
    """The set, the background and the parameters of one morphology step, checked."""
    if op in _MORPH_ADDS:
        s, bg, fill = _hole_set(kw)
    else:
        if kw.get('fill_label') is not None:
            raise ValueError('fill_label: erosion and opening add no voxel and take no fill_label')
        s, bg, fill = label_set(kw['labels_or_regions']), _integer(kw.get('background_label', 0), 'background_label'), 0
    iterations = _integer(kw.get('iterations', 1), 'iterations')
    if not 1 <= iterations <= 1024:
        raise ValueError(f'iterations must lie in 1..1024, got {iterations} (scipy\'s "below 1: until nothing changes" is not built)')
    conn = kw.get('connectivity', 6)
    if isinstance(conn, (bool, np.bool_)) or conn not in (6, 18, 26):
        raise ValueError(f'connectivity must be 6, 18 or 26, got {conn!r}')
    border = kw.get('border_value', 0)
    if border not in (0, 1):
        raise ValueError(f'border_value must be 0 or 1, got {border!r}')
    return s, bg, MorphParams(op, int(conn), iterations, int(border), fill)


def plan_passes(pp_fns: Sequence[Callable], pp_fn_kwargs: Sequence[dict]) -> List[Tuple]:
    """Group the steps into passes, in order: one entry per GPU call or host step.  Returns a list of

    * ``('gpu', [(S, background_label, step), ...])`` - one ``fnn_keep_largest_components`` call;
    * ``('gpu_small', [(S, background_label, step, min_size), ...])`` - one ``fnn_remove_small_components`` call, all of
      its steps with one connectivity (``pp_fn_kwargs[step]``'s); a ``per_member`` step gives one entry per member;
    * ``('gpu_holes', [(S, background_label, step, fill_label)])`` - one ``fnn_fill_holes`` call, always one step;
    * ``('gpu_morph', [(S, background_label, step, MorphParams)])`` - one ``fnn_binary_morphology`` call, always one step;
    * ``('host', step)`` - any other callable, on its own, on the host.

    A step joins the open pass of its own kind only if each of its sets is disjoint from every set already in it, it has
    the same ``background_label``, and that background is not in its own sets (otherwise voxels an earlier step of the
    pass set to background would belong to its mask).  The arguments of the new steps are checked here (ValueError)."""
    passes: List[Tuple] = []
    for k, (fn, kw) in enumerate(zip(pp_fns, pp_fn_kwargs)):
        kw = dict(kw)
        if fn is fill_holes_in_segmentation:
            s, bg, fill = _hole_set(kw)
            passes.append(('gpu_holes', [(s, bg, k, fill)]))
            continue
        op = next((code for f, code in _MORPH_OPS if fn is f), None)      # by identity: a host step need not be hashable
        if op is not None:
            s, bg, params = _morph_step(op, kw)
            passes.append(('gpu_morph', [(s, bg, k, params)]))
            continue
        if fn is remove_small_components_from_segmentation:
            sets, sizes, conn = _small_component_sets(kw)
            bg = _integer(kw.get('background_label', 0), 'background_label')
            cur = passes[-1] if passes and passes[-1][0] == 'gpu_small' else None
            if (cur is not None and pp_fn_kwargs[cur[1][0][2]].get('connectivity', 26) == conn and
                    all(bg not in s and all(bg == e[1] and not (s & e[0]) for e in cur[1]) for s in sets)):
                cur[1].extend((s, bg, k, m) for s, m in zip(sets, sizes))
            else:
                passes.append(('gpu_small', [(s, bg, k, m) for s, m in zip(sets, sizes)]))
            continue
        if not _is_ours(fn):
            passes.append(('host', k))
            continue
        s = label_set(kw['labels_or_regions'])
        bg = int(kw.get('background_label', 0))
        cur = passes[-1] if passes and passes[-1][0] == 'gpu' else None
        if cur is not None and bg not in s and all(bg == b and not (s & t) for t, b, _ in cur[1]):
            cur[1].append((s, bg, k))
        else:
            passes.append(('gpu', [(s, bg, k)]))
    return passes


class GpuPass(NamedTuple):
    """One GPU call of ``_run_passes``: which entry it is and what it takes."""
    call: str                                   # 'largest', 'small', 'holes' or 'morph'
    sets: List[frozenset]                       # disjoint label sets, all labelled in this call ('holes', 'morph': one)
    background: int
    min_size: Tuple[int, ...] = ()              # 'small': one per set
    connectivity: int = 26                      # 'small'; 'morph': 6, 18 or 26
    fill_label: int = 0                         # 'holes'; 'morph': the adding ops'
    op: int = 0                                 # 'morph': capi.FNN_MORPH_*
    iterations: int = 1                         # 'morph'
    border_value: int = 0                       # 'morph'


def _gpu_pass(kind: str, body, pp_fn_kwargs) -> GpuPass:
    """A GPU entry of ``plan_passes`` as the call ``_run_passes`` makes."""
    sets, bg = [e[0] for e in body], body[0][1]
    if kind == 'gpu_small':
        return GpuPass('small', sets, bg, tuple(e[3] for e in body), int(pp_fn_kwargs[body[0][2]].get('connectivity', 26)))
    if kind == 'gpu_holes':
        return GpuPass('holes', sets, bg, fill_label=body[0][3])
    if kind == 'gpu_morph':
        m = body[0][3]
        return GpuPass('morph', sets, bg, connectivity=m.connectivity, fill_label=m.fill_label, op=m.op, iterations=m.iterations,
                       border_value=m.border_value)
    return GpuPass('largest', sets, bg)


def _as_device_u(seg: torch.Tensor) -> Tuple[torch.Tensor, bool]:
    """A contiguous private copy the kernel can work on in place: uint8 stays uint8, anything else is carried as the
    bits of uint16 in int16 (values checked to lie in 0..65535)."""
    if seg.dtype == torch.uint8:
        return seg.clone(memory_format=torch.contiguous_format), False
    if seg.dtype == torch.bool or seg.dtype.is_floating_point or seg.dtype.is_complex:
        raise ValueError(f'label maps must have an integer dtype, got {seg.dtype}')
    if seg.numel():
        lo, hi = int(seg.min()), int(seg.max())
        if lo < 0 or hi > 65535:
            raise ValueError(f'label values must lie in 0..65535 (got {lo}..{hi})')
    return seg.to(torch.int32).to(torch.int16).contiguous(), True


def _check_passes(passes: Sequence[GpuPass], u16: bool):
    """The labels a pass writes must fit the map's dtype: a ValueError naming the argument, before any GPU call."""
    limit, name = (65536, 'uint16') if u16 else (256, 'uint8')
    for p in passes:
        if p.background < 0 or p.background >= limit:
            raise ValueError(f'background_label {p.background} does not fit the label map ({name})')
        fills = p.call == 'holes' or (p.call == 'morph' and p.op in _MORPH_ADDS)
        if fills and (p.fill_label < 0 or p.fill_label >= limit):
            raise ValueError(f'fill_label {p.fill_label} does not fit the label map ({name})')


def _run_passes(work: torch.Tensor, u16: bool, passes: Sequence[GpuPass], border_axes: int = 7):
    """Apply GPU passes in order to the [X, Y, Z] device tensor ``work`` (in place).  ``border_axes``: ``fnn_fill_holes``'s and
    ``fnn_binary_morphology``'s ``axes``, 6 for a 2-D map carried as [1, Y, Z]."""
    limit = 65536 if u16 else 256
    _check_passes(passes, u16)
    with torch.cuda.device(work.device):
        stream = torch.cuda.current_stream(work.device).cuda_stream
        for p in passes:
            top = max((max(s) for s in p.sets if s), default=-1)
            table = np.full(min(max(top + 1, 0), limit), -1, np.int32)
            for g, s in enumerate(p.sets):
                for v in s:
                    if 0 <= v < limit:
                        table[v] = g
            if p.call == 'largest':
                capi.keep_largest_components(work.data_ptr(), u16, work.shape, table, len(p.sets), p.background, stream)
            elif p.call == 'small':
                capi.remove_small_components(work.data_ptr(), u16, work.shape, table, len(p.sets), p.background, p.min_size,
                                             p.connectivity, stream)
            elif p.call == 'holes':
                capi.fill_holes(work.data_ptr(), u16, work.shape, table, p.background, p.fill_label, border_axes, stream)
            elif p.call == 'morph':
                capi.binary_morphology(work.data_ptr(), u16, work.shape, table, p.op, p.connectivity, p.iterations, p.border_value,
                                       p.background, p.fill_label, border_axes, stream)
            else:
                raise ValueError(f'unknown GPU pass {p.call!r}')


def _device_postprocess(seg: torch.Tensor, passes: Sequence[GpuPass]) -> torch.Tensor:
    """Device tensor (2-D or 3-D) -> new device tensor of the same dtype and shape."""
    if seg.ndim not in (2, 3):
        raise ValueError(f'segmentation must be 2-D or 3-D, got shape {tuple(seg.shape)}')
    work, u16 = _as_device_u(seg)
    work3 = work.view(1, *work.shape) if work.ndim == 2 else work
    _run_passes(work3, u16, passes, border_axes=6 if work.ndim == 2 else 7)
    if not u16:
        return work
    return as_plain_labels(work).to(seg.dtype)


def _device() -> torch.device:
    if not torch.cuda.is_available():
        raise RuntimeError('connected-component postprocessing runs on an AMD GPU through the HIP engine; no GPU is visible')
    return torch.device('cuda', torch.cuda.current_device())


def _postprocess(segmentation, passes: Sequence[GpuPass]):
    """numpy in -> numpy out (same dtype); torch in -> new torch tensor on the input's device (CUDA work either way).
    What can be refused from the arguments alone is refused before a GPU is asked for."""
    if isinstance(segmentation, torch.Tensor):
        _check_passes(passes, segmentation.dtype != torch.uint8)
        if segmentation.device.type == 'cuda':
            return _device_postprocess(segmentation, passes)
        out = _device_postprocess(segmentation.to(_device()), passes)
        return out.to(segmentation.device)
    arr = np.asarray(segmentation)
    if arr.dtype.kind not in 'iu':
        raise ValueError(f'label maps must have an integer dtype, got {arr.dtype}')
    if arr.size and (int(arr.min()) < 0 or int(arr.max()) > 65535):
        raise ValueError(f'label values must lie in 0..65535 (got {int(arr.min())}..{int(arr.max())})')
    _check_passes(passes, arr.dtype != np.uint8)
    if arr.dtype == np.uint8:
        t = torch.from_numpy(np.ascontiguousarray(arr))
    else:
        t = torch.from_numpy(np.ascontiguousarray(arr, dtype=np.int32))
    out = _device_postprocess(t.to(_device()), passes)
    return out.cpu().numpy().astype(arr.dtype, copy=False)


def remove_all_but_largest_component_from_segmentation(segmentation, labels_or_regions: Union[int, Tuple[int, ...],
                                                                                                List[Union[int, Tuple[int, ...]]]],
                                                       background_label: int = 0):
    """Reference signature (remove_connected_components.py:21-33).  ``segmentation``: numpy (returns numpy of the same
    dtype) or a torch tensor (returns a new tensor on its device), 2-D or 3-D, values 0..65535."""
    return _postprocess(segmentation, [GpuPass('largest', [label_set(labels_or_regions)], int(background_label))])


def _one_step(fn, segmentation, kw: dict):
    (kind, body), = plan_passes([fn], [kw])
    return _postprocess(segmentation, [_gpu_pass(kind, body, [kw])])


def remove_small_components_from_segmentation(segmentation, labels_or_regions, min_size, background_label: int = 0,
                                              connectivity: int = 26, per_member: bool = False):
    """Every connected component of the mask ``seg in S`` with fewer than ``min_size`` voxels becomes
    ``background_label``; one of exactly ``min_size`` voxels is kept, ``min_size <= 1`` changes nothing.  S is the union
    of ``labels_or_regions`` as in ``remove_all_but_largest_component_from_segmentation``; with a list and
    ``per_member=True`` each member is a set of its own (they must be disjoint; ``min_size`` may then be a sequence, one
    entry per member) and all of them are labelled on the input map in one pass.  ``connectivity``: 26 (8 in 2-D, a
    voxel's full neighbourhood) or 6 (4 in 2-D, face neighbours).  ``min_size`` counts voxels: for a size in physical
    units divide by the voxel volume first.  ``segmentation``, dtype and values: as the function above; the input is left alone."""
    return _one_step(remove_small_components_from_segmentation, segmentation,
                     dict(labels_or_regions=labels_or_regions, min_size=min_size, background_label=background_label,
                          connectivity=connectivity, per_member=per_member))


def fill_holes_in_segmentation(segmentation, labels_or_regions, fill_label: Optional[int] = None, background_label: int = 0):
    """scipy's ``binary_fill_holes`` of the mask ``seg in S`` (default structure; the whole volume for a 3-D map, the plane
    for a 2-D one): a hole is a face-connected part of the mask's complement that does not reach the border of the map.
    Hole voxels whose value is ``background_label`` become ``fill_label`` - by default the label of S when it has exactly
    one, otherwise it must be given - and any other label inside a hole (a tumour inside an organ) stays.
    ``segmentation``, dtype and values: as the functions above; the input is left alone."""
    return _one_step(fill_holes_in_segmentation, segmentation,
                     dict(labels_or_regions=labels_or_regions, fill_label=fill_label, background_label=background_label))


def binary_dilation_in_segmentation(segmentation, labels_or_regions, iterations: int = 1, connectivity: int = 6,
                                    border_value: int = 0, fill_label: Optional[int] = None, background_label: int = 0):
    """scipy's ``binary_dilation`` of the mask ``seg in S`` with ``generate_binary_structure(ndim, rank)`` - ``connectivity`` 6,
    18 or 26 is rank 1, 2 or 3; on a 2-D map 6 is the cross and 18 and 26 the full 3x3 - ``iterations`` times (1..1024), the
    outside of the map counting as ``border_value`` (0 or 1).  The voxels the mask gains whose value is ``background_label``
    become ``fill_label`` - by default the label of S when it has exactly one, otherwise it must be given - and any other
    label in the grown zone stays.  ``segmentation``, dtype and values: as the functions above; the input is left alone."""
    return _one_step(binary_dilation_in_segmentation, segmentation,
                     dict(labels_or_regions=labels_or_regions, iterations=iterations, connectivity=connectivity,
                          border_value=border_value, fill_label=fill_label, background_label=background_label))


def binary_closing_in_segmentation(segmentation, labels_or_regions, iterations: int = 1, connectivity: int = 6,
                                   border_value: int = 0, fill_label: Optional[int] = None, background_label: int = 0):
    """scipy's ``binary_closing`` of the mask ``seg in S``: ``iterations`` dilations, then as many erosions, structure and
    ``border_value`` as in ``binary_dilation_in_segmentation``.  Closing only adds here: the voxels the mask gains whose value is
    ``background_label`` become ``fill_label`` (default as above), any other label there stays, and no voxel of S changes -
    with ``border_value=0`` scipy's closing erodes the mask from the faces of the map, and those voxels stay what they are."""
    return _one_step(binary_closing_in_segmentation, segmentation,
                     dict(labels_or_regions=labels_or_regions, iterations=iterations, connectivity=connectivity,
                          border_value=border_value, fill_label=fill_label, background_label=background_label))


def binary_erosion_in_segmentation(segmentation, labels_or_regions, iterations: int = 1, connectivity: int = 6,
                                   border_value: int = 0, background_label: int = 0):
    """scipy's ``binary_erosion`` of the mask ``seg in S``, structure, ``iterations`` and ``border_value`` as in
    ``binary_dilation_in_segmentation``: the voxels the mask loses become ``background_label``; with ``border_value=0`` a set
    that touches a face of the map is eroded from that face too, with 1 it is not.  No voxel outside S changes."""
    return _one_step(binary_erosion_in_segmentation, segmentation,
                     dict(labels_or_regions=labels_or_regions, iterations=iterations, connectivity=connectivity,
                          border_value=border_value, background_label=background_label))


def binary_opening_in_segmentation(segmentation, labels_or_regions, iterations: int = 1, connectivity: int = 6,
                                   border_value: int = 0, background_label: int = 0):
    """scipy's ``binary_opening`` of the mask ``seg in S``: ``iterations`` erosions, then as many dilations (thin bridges and
    specks go, what is left comes back to its size).  Opening only removes here: the voxels the mask loses become
    ``background_label`` and no voxel outside S changes - with ``border_value=1`` scipy's opening grows the mask from the faces
    of the map, and those voxels are not added."""
    return _one_step(binary_opening_in_segmentation, segmentation,
                     dict(labels_or_regions=labels_or_regions, iterations=iterations, connectivity=connectivity,
                          border_value=border_value, background_label=background_label))


_MORPH_OPS = ((binary_dilation_in_segmentation, capi.FNN_MORPH_DILATE), (binary_erosion_in_segmentation, capi.FNN_MORPH_ERODE),
              (binary_opening_in_segmentation, capi.FNN_MORPH_OPEN), (binary_closing_in_segmentation, capi.FNN_MORPH_CLOSE))


def apply_postprocessing(segmentation, pp_fns: Sequence[Callable], pp_fn_kwargs: Sequence[dict]):
    """``apply_postprocessing`` (remove_connected_components.py:36-39): every step in order, consecutive steps of
    this module fused into one labelling pass where ``plan_passes`` allows it; a chain of this module's steps of any
    kind costs one upload and one download.  Other callables run as they are, on a host (numpy) copy."""
    is_torch = isinstance(segmentation, torch.Tensor)
    seg = segmentation
    gpu: List[GpuPass] = []                              # consecutive GPU passes: one upload / download for all of them

    def flush(seg):
        if gpu:
            seg = _postprocess(seg, list(gpu))
            gpu.clear()
        return seg

    for kind, body in plan_passes(pp_fns, pp_fn_kwargs):
        if kind != 'host':
            gpu.append(_gpu_pass(kind, body, pp_fn_kwargs))
            continue
        seg = flush(seg)
        host = seg.cpu().numpy() if isinstance(seg, torch.Tensor) else np.asarray(seg)
        res = np.asarray(pp_fns[body](np.copy(host), **pp_fn_kwargs[body]))
        seg = torch.from_numpy(res).to(segmentation.device) if is_torch else res
    seg = flush(seg)
    if seg is segmentation:              # no step: still a new array, like the reference's copies
        seg = segmentation.clone() if is_torch else np.copy(segmentation)
    return seg


class _RestrictedUnpickler(pickle.Unpickler):
    """Reads ``postprocessing.pkl`` without nnunetv2: the reference's function maps onto this module's, this module's own
    further steps load under this module's name, numpy scalars and dtypes may be rebuilt, every other global is refused."""
    _NUMPY = {('numpy', 'dtype'), ('numpy.core.multiarray', 'scalar'), ('numpy._core.multiarray', 'scalar')}

    def find_class(self, module, name):
        if (module, name) in (REFERENCE_NAME, (__name__, REFERENCE_NAME[1])):      # also a pkl written with this module
            return remove_all_but_largest_component_from_segmentation
        if module == __name__ and name in _OWN_STEPS:                              # this module's steps beyond the reference's
            return _OWN_STEPS[name]
        if (module, name) in self._NUMPY:
            return np.dtype if name == 'dtype' else _numpy_scalar
        raise pickle.UnpicklingError(f'postprocessing.pkl names a global that is not allowed: {module}.{name}')


_OWN_STEPS = {f.__name__: f for f in (remove_small_components_from_segmentation, fill_holes_in_segmentation, *(f for f, _ in _MORPH_OPS))}


def _numpy_scalar(dtype, data=None):
    """numpy's scalar reconstructor, limited to plain numeric dtypes."""
    dtype = np.dtype(dtype)
    if dtype.kind not in 'biuf' or data is None:
        raise pickle.UnpicklingError(f'numpy scalar of dtype {dtype} is not allowed in postprocessing.pkl')
    return np.frombuffer(data, dtype=dtype, count=1)[0]


def load_postprocessing_pkl(path_or_bytes) -> Tuple[List[Callable], List[dict]]:
    """``(pp_fns, pp_fn_kwargs)`` from a reference ``postprocessing.pkl`` (path or bytes)."""
    if isinstance(path_or_bytes, (bytes, bytearray)):
        data = bytes(path_or_bytes)
    else:
        with open(path_or_bytes, 'rb') as f:
            data = f.read()
    pp_fns, pp_fn_kwargs = _RestrictedUnpickler(io.BytesIO(data)).load()
    pp_fns, pp_fn_kwargs = list(pp_fns), [dict(k) for k in pp_fn_kwargs]
    if len(pp_fns) != len(pp_fn_kwargs):
        raise pickle.UnpicklingError('postprocessing.pkl: as many kwargs as functions expected')
    return pp_fns, pp_fn_kwargs


def determine_postprocessing(predictions, references, dataset_json_or_label_manager, output_folder=None,
                             save_postprocessed=False, verbose=False, backend=None):
    """``determine_postprocessing`` (remove_connected_components.py:52-245) on label maps, on the GPU; see
    ``postprocessing_search.determine_postprocessing``."""
    from .postprocessing_search import determine_postprocessing as run
    return run(predictions, references, dataset_json_or_label_manager, output_folder, save_postprocessed, verbose, backend)


# ---- label files ---------------------------------------------------------------------------------------------------------
def _compressor(rw, compress_on_device):
    """``compress_on_device`` (False, True or ``'dynamic'``; anything else a ValueError) -> ``labels_for_writer``'s ``compress``."""
    mode = compress_mode(compress_on_device)
    if mode == 'dynamic':
        return functools.partial(rw.compress_labels, tables='dynamic')
    return rw.compress_labels if mode else None


def _postprocessed_for_writer(rw, labels, props, pp_fns, pp_fn_kwargs, compress):
    """The GPU part of one file: decoded labels -> what ``rw.write_seg`` takes on a thread that makes no GPU call."""
    seg = apply_postprocessing(as_plain_labels(labels), pp_fns, pp_fn_kwargs)
    return labels_for_writer(rw, seg, props, compress=compress)


def load_postprocess_save(segmentation_file: str, output_fname: str, image_reader_writer, pp_fns: Sequence[Callable],
                          pp_fn_kwargs: Sequence[dict], compress_on_device=False):
    """``load_postprocess_save`` (remove_connected_components.py:42-50): the file is read as labels on the device,
    post-processed there and written with its own properties.  ``compress_on_device``: False, True or ``'dynamic'``."""
    compress = _compressor(image_reader_writer, compress_on_device)
    labels, props = image_reader_writer.read_label_map(segmentation_file)
    out = _postprocessed_for_writer(image_reader_writer, labels, props, pp_fns, pp_fn_kwargs, compress)
    image_reader_writer.write_seg(out, output_fname, props)


def apply_postprocessing_to_files(input_files: Sequence[str], output_files: Sequence[str], image_reader_writer,
                                  pp_fns: Sequence[Callable], pp_fn_kwargs: Sequence[dict], compress_on_device=False):
    """``load_postprocess_save`` for every pair of names, pipelined: a reader thread inflates the next file and a writer
    thread compresses and writes the previous one while the calling thread - the only one that touches the GPU - decodes
    and post-processes this one.  A file appears under its name only when it is complete."""
    from .label_folders import run_label_cases
    rw = image_reader_writer
    input_files, output_files = list(input_files), list(output_files)
    compress = _compressor(rw, compress_on_device)

    def run(i, maps):
        labels, props = maps[0]
        out = _postprocessed_for_writer(rw, labels, props, pp_fns, pp_fn_kwargs, compress)
        return None, (lambda: rw.write_seg(out, output_files[i], props))

    run_label_cases(rw, [[f] for f in input_files], run, write_thread=True)


def apply_postprocessing_to_folder(input_folder: str, output_folder: str, pp_fns: Sequence[Callable], pp_fn_kwargs: Sequence[dict],
                                   plans_file_or_dict=None, dataset_json_file_or_dict=None, num_processes=8,
                                   compress_on_device=False, inflate_on_device=False) -> None:
    """``apply_postprocessing_to_folder`` (remove_connected_components.py:247-294).  If plans_file_or_dict or
    dataset_json_file_or_dict are None, they are looked for in input_folder.  ``num_processes`` is accepted and ignored;
    ``compress_on_device`` (True, or ``'dynamic'`` for per-chunk Huffman tables; anything but those and False is a
    ValueError before any file is read) writes the ``.nii.gz`` files through ``compress_labels`` (no label map is downloaded);
    ``inflate_on_device`` reads input files that were written that way through ``fnn_inflate_segments`` (no zlib on the host);
    ``inflate_on_device='dynamic'`` through ``fnn_inflate_segments_dyn``, which serves files written with
    ``compress_on_device='dynamic'`` too."""
    from .label_folders import folder_plans_and_dataset, subfiles
    compress_mode(compress_on_device)
    _, dataset_json, rw = folder_plans_and_dataset(
        input_folder, plans_file_or_dict, dataset_json_file_or_dict,
        'Expected plans file missing: {}. The plans file should have been created while running nnUNetv2_predict. Sadge. '
        'If the folder you want to apply postprocessing to was create from an ensemble then just specify one of the '
        'plans files of the ensemble members in plans_file_or_dict',
        'Expected plans file missing: {}. The dataset.json should have been copied while running '
        'nnUNetv2_predict/nnUNetv2_ensemble. Sadge.', inflate_on_device=inflate_on_device)
    os.makedirs(output_folder, exist_ok=True)
    files = subfiles(input_folder, suffix=dataset_json['file_ending'], join=False)
    apply_postprocessing_to_files([os.path.join(input_folder, i) for i in files], [os.path.join(output_folder, i) for i in files],
                                  rw, pp_fns, pp_fn_kwargs, compress_on_device)


def determine_postprocessing_on_folder(folder_predictions: str, folder_ref: str, plans_file_or_dict=None,
                                       dataset_json_file_or_dict=None, num_processes: int = 8,
                                       keep_postprocessed_files: bool = True, inflate_on_device=False):
    """The reference's ``determine_postprocessing`` (remove_connected_components.py:52-244) on folders of label files; see
    ``postprocessing_search.determine_postprocessing_on_folder``."""
    from .postprocessing_search import determine_postprocessing_on_folder as run
    return run(folder_predictions, folder_ref, plans_file_or_dict, dataset_json_file_or_dict, num_processes,
               keep_postprocessed_files, inflate_on_device=inflate_on_device)
