"""What the folder front-ends share on top of ``case_pipeline``: its loop over cases that are label files, where a folder's
plans, dataset.json and reader-writer come from, and the few file-system helpers of the reference they need.
"""
from __future__ import annotations

import json
import os
from typing import Callable, List, Optional, Sequence

from .case_pipeline import run_pipeline


def subfiles(folder: str, suffix: Optional[str] = None, join: bool = True) -> List[str]:
    """batchgenerators' ``subfiles(folder, suffix=..., join=...)``: the sorted files of ``folder`` that end with ``suffix``."""
    names = sorted(i for i in os.listdir(folder)
                   if os.path.isfile(os.path.join(folder, i)) and (suffix is None or i.endswith(suffix)))
    return [os.path.join(folder, i) for i in names] if join else names


def load_json(path: str):
    with open(path) as f:
        return json.load(f)


def run_label_cases(rw, cases: Sequence[Sequence[str]], run: Callable, write_thread: bool = False) -> list:
    """``run_pipeline`` over cases that are lists of label files: ``run(i, maps)`` gets what ``rw.decode_label_maps`` makes
    of case i - per file ``(device labels (z, y, x), properties)``.  Two slots of pinned staging buffers alternate."""
    def stage(i):
        return rw.stage_label_files(cases[i], slot=i % 2).fill

    return run_pipeline(len(cases), stage, lambda i, staged: run(i, rw.decode_label_maps(staged)), write_thread=write_thread)


def folder_plans_and_dataset(folder: str, plans_file_or_dict=None, dataset_json_file_or_dict=None,
                             missing_plans: Optional[str] = None, missing_dataset: Optional[str] = None,
                             inflate_on_device=False):
    """Plans and dataset.json as given (a dict or a file name), or looked for in ``folder`` -> (PlansManager, dataset.json,
    an instance of the reader-writer they name).  ``missing_*``: the caller's RuntimeError text for a file that is not in
    the folder, ``{}`` standing for its name (None: opening it raises).  ``inflate_on_device``: the reader-writer inflates
    label files written with ``compress_on_device=True`` on the GPU (``NiftiIO(inflate_on_device=True)``), with ``'dynamic'``
    those written with ``compress_on_device='dynamic'`` too (``NiftiIO(inflate_on_device='dynamic')``), with ``'any'`` every
    single-member ``.nii.gz`` label file, whoever wrote it (``NiftiIO(inflate_on_device='any')``)."""
    from .imageio import prediction_reader_writer_class
    from .plans import PlansManager

    def given_or_found(given, name, missing):
        if given is None:
            given = os.path.join(folder, name)
            if missing is not None and not os.path.isfile(given):
                raise RuntimeError(missing.format(given))
        return given if isinstance(given, dict) else load_json(given)

    plans_manager = PlansManager(given_or_found(plans_file_or_dict, 'plans.json', missing_plans))
    dataset_json = given_or_found(dataset_json_file_or_dict, 'dataset.json', missing_dataset)
    return plans_manager, dataset_json, prediction_reader_writer_class(plans_manager, dataset_json)(inflate_on_device=inflate_on_device)
