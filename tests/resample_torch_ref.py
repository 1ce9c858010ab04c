"""nnU-Net's torch resampling family (``resample_torch_fornnunet``) restated on top of
``torch.nn.functional.interpolate`` on the CPU - the operator the reference itself calls, so torch is the yardstick
of ``tests/test_gpu_resample_torch.py``; ``tests/golden/resample_torch.npz`` (made by the reference's own functions)
pins this restatement in ``tests/test_resample_torch_cpu.py``.

* images / logits: ``interpolate(x[None].float(), size, mode='trilinear', antialias=False)``;
* separate-z: bilinear per slice of the axis, then ``mode='nearest-exact'`` to the full shape.  (The reference's branch
  raises a TypeError before it gets there - ``len()`` of an integer axis; this is what the branch states.)
* segmentations: per unique label u ascending the score ``interpolate((seg == u) * 1000)`` stored as fp16; above 700 the
  voxel takes u, the rest take the first maximum over the scores.  ``memefficient``: float32 score of ``(seg == u)``
  above 0.5 takes u (later labels overwrite), else 0.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F


def _interp(x: torch.Tensor, size, mode: str) -> torch.Tensor:
    """x [C, *spatial] -> [C, *size]; 'linear' is bi-/trilinear by rank, as the reference picks it."""
    if mode == 'linear':
        mode = {3: 'bilinear', 4: 'trilinear'}[x.ndim]
    kw = {} if mode.startswith('nearest') else {'antialias': False}
    return F.interpolate(x[None], tuple(int(i) for i in size), mode=mode, **kw)[0]


def _labels_from_scores(values: torch.Tensor, scores: torch.Tensor, memefficient: bool) -> torch.Tensor:
    """scores [U, ...] of the ascending unique ``values`` -> int16 labels by the reference's two rules."""
    if memefficient:
        out = torch.zeros(scores.shape[1:], dtype=torch.int16)
        for i, u in enumerate(values.tolist()):
            out[scores[i] > 0.5] = u
        return out
    out = values[scores.argmax(0)].to(torch.int16)            # first maximum; a score above 700 is the maximum
    for i, u in enumerate(values.tolist()):
        out[scores[i] > 700] = u
    return out


def _simple(x: torch.Tensor, size, is_seg: bool, memefficient: bool, mode: str) -> torch.Tensor:
    """One call of the reference's inner function: x [C, *spatial] -> [C, *size]."""
    if [int(i) for i in size] == [int(i) for i in x.shape[1:]]:
        return x
    if not is_seg:
        return _interp(x if x.dtype == torch.float64 else x.float(), size, mode)
    values = torch.unique(x)
    if memefficient:
        scores = torch.stack([_interp((x == u).float(), size, mode) for u in values])
    else:
        scores = torch.stack([_interp((x == u).float() * 1000, size, mode).half() for u in values])
    return _labels_from_scores(values, scores, memefficient)


def _fold(x: torch.Tensor, axis: int) -> torch.Tensor:
    """[C, x, y, z] -> [(C, axis), the two other axes]."""
    return x.movedim(1 + axis, 1).reshape(-1, *[x.shape[1 + a] for a in range(3) if a != axis])


def _unfold(x: torch.Tensor, axis: int, c: int) -> torch.Tensor:
    return x.reshape(c, -1, *x.shape[1:]).movedim(1, 1 + axis)


def resample(x, new_shape, separate_axis=None, is_seg: bool = False, memefficient: bool = False) -> torch.Tensor:
    """``resample_torch_fornnunet`` with the decision (``separate_axis``) already taken: float32 for images, int16 for
    segmentations.  A float64 image stays float64: the same operator in exact-enough arithmetic, against which the
    float32 operator's own error is measured."""
    x = torch.as_tensor(np.asarray(x)) if not isinstance(x, torch.Tensor) else x.cpu()
    new_shape = [int(i) for i in new_shape]
    if separate_axis is None:
        out = _simple(x, new_shape, is_seg, memefficient, 'linear')
    else:
        plane = [new_shape[a] for a in range(3) if a != separate_axis]
        y = _unfold(_simple(_fold(x, separate_axis), plane, is_seg, memefficient, 'linear'), separate_axis, x.shape[0])
        out = _simple(y, new_shape, is_seg, memefficient, 'nearest-exact')
    if is_seg:
        return out.to(torch.int16)
    return out if out.dtype == torch.float64 else out.float()


def seg_scores(seg, new_shape, separate_axis=None, memefficient: bool = False):
    """-> (ascending unique labels [U], scores [U, C, *new_shape]) behind ``resample(is_seg=True)``: fp16 scores of
    ``(seg == u) * 1000`` as float32, or the float32 scores of ``(seg == u)`` for ``memefficient``.  Along a separate
    axis the nearest-exact pass only picks slices, so it is applied to the scores."""
    seg = torch.as_tensor(np.asarray(seg)) if not isinstance(seg, torch.Tensor) else seg.cpu()
    new_shape = [int(i) for i in new_shape]
    values = torch.unique(seg)
    out = []
    for u in values:
        m = (seg == u).float() * (1 if memefficient else 1000)
        if separate_axis is None:
            s = _simple(m, new_shape, False, False, 'linear')
        else:
            plane = [new_shape[a] for a in range(3) if a != separate_axis]
            s = _unfold(_simple(_fold(m, separate_axis), plane, False, False, 'linear'), separate_axis, m.shape[0])
        s = s if memefficient else s.half().float()
        out.append(_simple(s, new_shape, False, False, 'nearest-exact') if separate_axis is not None else s)
    return values, torch.stack(out)


def labels_from_scores(values, scores, memefficient: bool = False) -> torch.Tensor:
    return _labels_from_scores(values, scores, memefficient)


def check_labels(got, values, scores, memefficient):
    """``got`` against the yardstick's ``scores`` [U, ...] of ``values``: equal to the yardstick's label except at
    near-ties, where it must be one of the yardstick's two best; -> (excluded share, mismatches outside)."""
    want = _labels_from_scores(values, scores, memefficient).numpy()
    got = np.asarray(got)
    if memefficient:
        best = scores.max(0).values
        tie = ((best - 0.5).abs() <= 2.0 ** -20).numpy()
        # at a tie the voxel is the best-scoring label or 0
        allowed = (got == values[scores.argmax(0)].numpy()) | (got == 0)
    else:
        top = scores.topk(min(2, scores.shape[0]), dim=0)
        tie = ((top.values[0] - top.values[-1]) <= 0.5).numpy() & (scores.shape[0] > 1)
        allowed = np.zeros(got.shape, bool)
        for k in range(top.indices.shape[0]):
            allowed |= got == values[top.indices[k]].numpy()
    share = float(tie.mean())
    assert share <= 0.02, f'near-ties are {share:.4f} of the case: choose smoother labels / another ratio'
    bad = int(((got != want) & ~tie).sum())
    assert bad == 0, f'{bad} labels differ away from near-ties'
    assert bool(allowed[tie].all()), 'a near-tie voxel took a label that is not one of the two best'
    return share, int((got != want).sum())


def blobby_labels(shape, values, seed: int, coarse=(4, 5, 4)) -> np.ndarray:
    """A smooth label map [1, *shape] (int16) over ``values``: the argmax of coarse random fields enlarged to ``shape`` -
    connected regions with smooth borders, like a segmentation and unlike white noise."""
    g = torch.Generator().manual_seed(int(seed))
    fields = torch.randn(len(values), *coarse, generator=g)
    big = F.interpolate(fields[None], tuple(int(i) for i in shape), mode='trilinear', align_corners=True)[0]
    idx = big.argmax(0).numpy()
    return np.asarray(values, dtype=np.int16)[idx][None]
