#!/usr/bin/env python3
"""Generate ``ensemble.npz`` FROM THE REFERENCE ITSELF (build container only: needs the reference's sources).

    python tests/golden/make_golden_ensemble.py

Every case is a small ensemble: each member's probabilities are made by the reference's
``convert_predicted_logits_to_segmentation_with_correct_shape(..., return_probabilities=True)`` from seeded fp16 logits
of the cropped grid (so they carry the crop box and ``transpose_backward`` of the case), written to an ``.npz`` file the
way nnU-Net exports them, and then handed to the reference's ``average_probabilities`` and
``LabelManager.convert_logits_to_segmentation`` - what ``merge_files`` does.  Stored per case: the members'
probabilities (the inputs), the average and the labels.  Data only; no reference source travels.
"""
from __future__ import annotations

import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import ref_shims  # noqa: E402

ref_shims.install()

from nnunetv2.ensembling.ensemble import average_probabilities  # noqa: E402
from nnunetv2.inference.export_prediction import convert_predicted_logits_to_segmentation_with_correct_shape  # noqa: E402
from nnunetv2.utilities.plans_handling.plans_handler import PlansManager  # noqa: E402

from golden_cases import DATASET_JSONS  # noqa: E402

# name, dataset, members, cropped, bbox (transposed axes), shape_before_cropping (transposed), transpose_forward
ENSEMBLE_CASES = [
    dict(name='labels_2_transposed', dataset='two_mod', members=2, cropped=(10, 12, 9), bbox=[[2, 12], [1, 13], [3, 12]],
         before=(14, 15, 13), tf=(2, 0, 1), seed=11),
    dict(name='labels_4_crop', dataset='labels3', members=4, cropped=(6, 7, 8), bbox=[[1, 7], [0, 7], [2, 10]],
         before=(8, 7, 12), tf=(1, 2, 0), seed=12),
    dict(name='regions_3_crop', dataset='regions', members=3, cropped=(8, 9, 10), bbox=[[0, 8], [2, 11], [1, 11]],
         before=(8, 12, 11), tf=(0, 2, 1), seed=13),
]


def member_logits(case, heads, m):
    rng = np.random.default_rng(7000 + 100 * case['seed'] + m)
    x = (rng.standard_normal((heads, *case['cropped'])) * 3).astype(np.float16)
    x[:, 0, 0, :2] = x[0, 0, 0, 0]                        # every head equal: exact ties the first maximum wins
    return x


def main():
    arrays = {}
    with tempfile.TemporaryDirectory() as tmp:
        for case in ENSEMBLE_CASES:
            dj = DATASET_JSONS[case['dataset']]
            tf = list(case['tf'])
            tb = [int(i) for i in np.argsort(tf)]
            plans = {'dataset_name': 'Dataset997_Ensemble', 'plans_name': 'nnUNetPlans', 'transpose_forward': tf,
                     'transpose_backward': tb, 'label_manager': 'LabelManager',
                     'configurations': {'3d_fullres': {
                         'patch_size': [8, 8, 8], 'spacing': [1.0, 1.0, 1.0],
                         'resampling_fn_probabilities': 'resample_data_or_seg_to_shape',
                         'resampling_fn_probabilities_kwargs': {'is_seg': False, 'order': 1, 'order_z': 0,
                                                                'force_separate_z': None},
                         'architecture': {'network_class_name': 'x', 'arch_kwargs': {}, '_kw_requires_import': []}}}}
            pm = PlansManager(plans)
            cm = pm.get_configuration('3d_fullres')
            lm = pm.get_label_manager(dj)
            props = {'spacing': [1.0, 1.0, 1.0], 'shape_before_cropping': tuple(case['before']),
                     'bbox_used_for_cropping': [list(b) for b in case['bbox']],
                     'shape_after_cropping_and_before_resampling': tuple(case['cropped'])}
            files = []
            for m in range(case['members']):
                _, probs = convert_predicted_logits_to_segmentation_with_correct_shape(
                    torch.from_numpy(member_logits(case, lm.num_segmentation_heads, m)), pm, cm, lm, props,
                    return_probabilities=True)
                probs = np.asarray(probs, dtype=np.float32)
                f = os.path.join(tmp, f"{case['name']}_{m}.npz")
                np.savez_compressed(f, probabilities=probs)
                files.append(f)
                arrays[f"{case['name']}__member{m}"] = probs
            avg = average_probabilities(files)
            seg = lm.convert_logits_to_segmentation(avg)
            arrays[case['name'] + '__avg'] = np.asarray(avg)
            arrays[case['name'] + '__seg'] = np.asarray(seg)
    np.savez_compressed(os.path.join(HERE, 'ensemble.npz'), **arrays)
    print('ensemble', {k: (v.shape, str(v.dtype)) for k, v in arrays.items()})


if __name__ == '__main__':
    main()
