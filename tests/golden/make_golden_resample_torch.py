#!/usr/bin/env python3
"""Generate ``resample_torch.npz`` FROM THE REFERENCE ITSELF (build container only: needs the reference's sources).

    python tests/golden/make_golden_resample_torch.py

Small seeded inputs through the reference's own ``resample_torch_fornnunet`` (its non-separate branch: an image and a
label map under both segmentation rules) and through ``resample_torch_simple`` called the way the separate-z branch
states it - per slice of the axis with ``mode='linear'``, then ``mode='nearest-exact'`` to the full shape - because that
branch itself raises a TypeError (``len()`` of the integer axis) before it computes anything.  Stored per case: the
input, the target shape and the reference's output.  Data only; no reference source travels.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import ref_shims  # noqa: E402

ref_shims.install()

from nnunetv2.preprocessing.resampling.resample_torch import resample_torch_fornnunet, resample_torch_simple  # noqa: E402

from resample_torch_ref import blobby_labels  # noqa: E402

IN_SHAPE, NEW_SHAPE = (9, 20, 17), (12, 27, 15)
LABEL_SETS = {'few': (0, 1, 2, 3), 'sparse': (0, 3, 7, 200)}


def separate_branch(x: torch.Tensor, new_shape, axis: int, **kw) -> torch.Tensor:
    """The two ``resample_torch_simple`` calls of the reference's separate-z branch."""
    others = [a for a in range(3) if a != axis]
    folded = x.movedim(1 + axis, 1).reshape(-1, *[x.shape[1 + a] for a in others])
    y = resample_torch_simple(folded, [new_shape[a] for a in others], mode='linear', **kw)
    y = y.reshape(x.shape[0], x.shape[1 + axis], *y.shape[1:]).movedim(1, 1 + axis)
    return resample_torch_simple(y, list(new_shape), mode='nearest-exact', **kw)


def main():
    arrays = {'new_shape': np.asarray(NEW_SHAPE, np.int64)}
    iso = (1.0, 1.0, 1.0)
    img = torch.randn(2, *IN_SHAPE, generator=torch.Generator().manual_seed(2024)) * 3
    arrays['image__in'] = img.numpy()
    arrays['image__out'] = np.asarray(resample_torch_fornnunet(img, NEW_SHAPE, iso, iso, is_seg=False,
                                                               force_separate_z=False), np.float32)
    for axis in range(3):
        arrays[f'image__sep{axis}'] = np.asarray(separate_branch(img, NEW_SHAPE, axis, is_seg=False), np.float32)
    for name, values in LABEL_SETS.items():
        seg = torch.from_numpy(blobby_labels(IN_SHAPE, values, seed=len(values) + sum(values)))
        arrays[f'seg_{name}__in'] = seg.numpy()
        for memeff in (False, True):
            tag = 'memeff' if memeff else 'argmax'
            out = resample_torch_fornnunet(seg, NEW_SHAPE, iso, iso, is_seg=True, force_separate_z=False,
                                           memefficient_seg_resampling=memeff)
            arrays[f'seg_{name}__{tag}'] = np.asarray(out).astype(np.int16)
            for axis in range(3):
                out = separate_branch(seg, NEW_SHAPE, axis, is_seg=True, memefficient_seg_resampling=memeff)
                arrays[f'seg_{name}__{tag}_sep{axis}'] = np.asarray(out).astype(np.int16)
    # the branch that cannot run, recorded so that the note in the docstrings stays true of the reference
    try:
        resample_torch_fornnunet(img, NEW_SHAPE, (5.0, 1.0, 1.0), (3.5, 0.7, 1.2))
        arrays['separate_branch_raises'] = np.asarray(0)
    except TypeError:
        arrays['separate_branch_raises'] = np.asarray(1)
    np.savez_compressed(os.path.join(HERE, 'resample_torch.npz'), **arrays)
    print('resample_torch', {k: (v.shape, str(v.dtype)) for k, v in arrays.items()})


if __name__ == '__main__':
    main()
