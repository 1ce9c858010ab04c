"""``JHUPredictor``: the reference's second way out of the predictor (distillation/nnunetv2/inference/JHU_inference.py), which
writes one binary mask file per foreground label instead of a label map - the AbdomenAtlas / TotalSegmentator layout:

    <output_file_truncated>/predictions/<label_name><file_ending>        uint8, (seg == label)

``output_file_truncated`` is read as a folder, as ``export_prediction_from_logits_singleFiles`` (:21-64) reads it; no combined
label file is written; with ``save_probabilities`` the ``.npz`` and ``.pkl`` are written next to the folder as always.
Everything before the export is ``nnUNetPredictor``'s: the label map is made, postprocessed and brought to the file's frame
once, and only then split into masks.

* default: the label map is downloaded once and the writer thread writes every mask with ``write_seg((seg == l).astype(
  uint8), ...)`` - byte for byte the file the reference's call makes through this package's writer.
* ``compress_on_device=True`` and a ``.nii.gz`` ending: ``NiftiIO.compress_label_masks`` encodes all masks on the GPU in one
  pass (csrc/deflate_masks.hip) on the calling thread and the writer thread only assembles and writes the files - the same
  headers and voxels behind another deflate stream.

A region-based dataset is refused when the predictor is initialised: the reference's function keys a dict by the label
value, which is a list there, and cannot serve those datasets either.
"""
from __future__ import annotations

import os
from typing import List, Tuple

import numpy as np
import torch

from .predictor import nnUNetPredictor


def mask_file_names(label_manager, dataset_json: dict, output_file_truncated: str) -> List[Tuple[int, str]]:
    """-> [(label, <output_file_truncated>/predictions/<label_name><file_ending>)] for the foreground labels, in their order."""
    if label_manager.has_regions:
        raise NotImplementedError('per-label mask files are written for datasets with plain labels, not for region-based ones')
    name_of = {j: i for i, j in label_manager.label_dict.items()}
    folder = os.path.join(output_file_truncated, 'predictions')
    return [(int(l), os.path.join(folder, name_of[l] + dataset_json['file_ending'])) for l in label_manager.foreground_labels]


class JHUPredictor(nnUNetPredictor):
    def _build_engine(self):
        if self.label_manager.has_regions:                      # (before any GPU work)
            raise NotImplementedError('JHUPredictor writes one mask file per label of a dataset with plain labels; '
                                      'region-based datasets are not served (neither by the reference\'s export)')
        super()._build_engine()

    def _masks_on_device(self, rw) -> bool:
        return self.compress_on_device and hasattr(rw, 'compress_label_masks') \
            and str(self.dataset_json['file_ending']).lower().endswith('.nii.gz')

    def _labels_out(self, labels: torch.Tensor, u16: bool, props: dict, for_file: bool):
        """As ``nnUNetPredictor._labels_out`` (the label map on the host, in the file's frame where the reader-writer
        reorients); on the device route the list of compressed masks, one per foreground label."""
        rw = self._reader_writer() if for_file else None
        if rw is None or not self._masks_on_device(rw):
            return super()._labels_out(labels, u16, props, for_file)     # (which compresses under the same condition only)
        if self._postprocessing is not None:
            from .postprocessing import apply_postprocessing
            labels = apply_postprocessing(labels, *self._postprocessing)
        labels = labels.to(torch.int16) if u16 else labels.to(torch.uint8)
        return rw.compress_label_masks(labels, list(self.label_manager.foreground_labels), props)

    def _write_label_files(self, seg, props: dict, output_file_truncated: str):
        """Host only: the writer thread's part.  ``seg``: the list ``compress_label_masks`` made, or the label map (a numpy
        array in the frame ``write_seg`` expects, or ``FileFrameLabels``)."""
        from .imageio import FileFrameLabels
        rw = self._reader_writer()
        names = mask_file_names(self.label_manager, self.dataset_json, output_file_truncated)
        os.makedirs(os.path.join(output_file_truncated, 'predictions'), exist_ok=True)
        for i, (label, fname) in enumerate(names):
            if isinstance(seg, list):
                mask = seg[i]
            elif isinstance(seg, FileFrameLabels):
                mask = FileFrameLabels((seg.voxels == label).astype(np.uint8, copy=False), seg.affine)
            else:
                mask = (seg == label).astype(np.uint8, copy=False)
            rw.write_seg(mask, fname, props)
