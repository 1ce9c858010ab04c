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
  headers and voxels behind another deflate stream.  ``compress_on_device='dynamic'`` is refused when the predictor is made:
  the mask encoder writes the fixed Huffman code only.

A region-based dataset is refused when the predictor is initialised: the reference's function keys a dict by the label
value, which is a list there, and cannot serve those datasets either.
"""
from __future__ import annotations

import os
from typing import List, Tuple

import numpy as np

from .case_pipeline import device_compressor
from .predictor import nnUNetPredictor


def mask_file_names(label_manager, dataset_json: dict, output_file_truncated: str) -> List[Tuple[int, str]]:
    """-> [(label, <output_file_truncated>/predictions/<label_name><file_ending>)] for the foreground labels, in their order."""
    if label_manager.has_regions:
        raise NotImplementedError('per-label mask files are written for datasets with plain labels, not for region-based ones')
    name_of = {j: i for i, j in label_manager.label_dict.items()}
    folder = os.path.join(output_file_truncated, 'predictions')
    return [(int(l), os.path.join(folder, name_of[l] + dataset_json['file_ending'])) for l in label_manager.foreground_labels]


class JHUPredictor(nnUNetPredictor):
    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        if self.compress_on_device == 'dynamic':                # (before any case runs)
            raise NotImplementedError("JHUPredictor(compress_on_device='dynamic'): compress_label_masks, the per-label mask encoder "
                                      "(csrc/deflate_masks.hip), writes the fixed Huffman code only; use compress_on_device=True")

    def _build_engine(self):
        if self.label_manager.has_regions:                      # (before any GPU work)
            raise NotImplementedError('JHUPredictor writes one mask file per label of a dataset with plain labels; '
                                      'region-based datasets are not served (neither by the reference\'s export)')
        super()._build_engine()

    def _label_files(self, rw):
        """One mask file per foreground label: on the device route ``labels_for_writer`` makes the list of compressed masks
        (else the label map, as ``nnUNetPredictor`` hands it over) and ``_write_masks`` writes either."""
        masks = device_compressor(rw, self.compress_on_device, self.dataset_json['file_ending'], 'compress_label_masks')
        labels = list(self.label_manager.foreground_labels)
        return (None if masks is None else lambda seg, props: masks(seg, labels, props)), self._write_masks

    def _write_masks(self, seg, props: dict, output_file_truncated: str):
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
