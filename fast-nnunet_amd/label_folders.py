"""What the folder front-ends share: the case pipeline of ``predict_from_files`` for label files, and the few file-system
helpers of the reference they need.

``evaluation.compute_metrics_on_folder``, ``postprocessing.apply_postprocessing_to_folder``,
``postprocessing.determine_postprocessing_on_folder`` and ``ensembling.ensemble_folders`` all walk a list of cases the same
way: the calling thread is the only one that touches the GPU; one ``_HostWorker`` reads (and inflates) the files of case
i + 1 while case i runs; where files are written, a second one writes those of case i - 1.  No process is started.
"""
from __future__ import annotations

import json
import os
from typing import Callable, List, Optional, Sequence


def subfiles(folder: str, suffix: Optional[str] = None, join: bool = True) -> List[str]:
    """batchgenerators' ``subfiles(folder, suffix=..., join=...)``: the sorted files of ``folder`` that end with ``suffix``."""
    names = sorted(i for i in os.listdir(folder)
                   if os.path.isfile(os.path.join(folder, i)) and (suffix is None or i.endswith(suffix)))
    return [os.path.join(folder, i) for i in names] if join else names


def load_json(path: str):
    with open(path) as f:
        return json.load(f)


def run_pipeline(n_cases: int, stage: Callable, run: Callable, write_thread: bool = False) -> list:
    """The loop of ``nnUNetPredictor._predict_cases`` for any per-case work.

    ``stage(i)`` runs on the calling thread (it may allocate pinned memory) and returns a host-only callable that reads case
    i - run on the reader thread, its value handed to ``run``.  ``run(i, data)`` runs on the calling thread (the GPU part)
    and returns ``(result, export)``: ``export`` is None or a host-only callable that writes the case's files, run on the
    writer thread; at most one case waits for the disk.  Returns the results.  A failing case raises here, in the calling
    thread, after both threads have been joined."""
    from .predictor import _HostWorker
    results = []
    if n_cases == 0:
        return results
    reader = _HostWorker('fnn-reader')
    writer = _HostWorker('fnn-writer') if write_thread else None

    try:
        nxt = reader.submit(stage(0))
        pending = None                                           # the writer's job for the previous case
        for i in range(n_cases):
            data = nxt.result()                                  # case i is in host memory (or its read failed)
            # case i + 1 is read while case i runs; its slot's buffers were released when case i - 1 was decoded
            nxt = reader.submit(stage(i + 1)) if i + 1 < n_cases else None
            result, export = run(i, data)
            results.append(result)
            if export is None:
                continue
            if pending is not None:
                pending.result()
            pending = writer.submit(export) if writer is not None else export()
        if pending is not None:
            pending.result()
    finally:
        for w in (reader, writer):
            if w is not None:
                w.close()
    return results


def run_label_cases(rw, cases: Sequence[Sequence[str]], run: Callable, write_thread: bool = False) -> list:
    """``run_pipeline`` over cases that are lists of label files: ``run(i, maps)`` gets what ``rw.decode_label_maps`` makes
    of case i - per file ``(device labels (z, y, x), properties)``.  Two slots of pinned staging buffers alternate."""
    def stage(i):
        return rw.stage_label_files(cases[i], slot=i % 2).fill

    return run_pipeline(len(cases), stage, lambda i, staged: run(i, rw.decode_label_maps(staged)), write_thread=write_thread)


def as_plain_labels(labels):
    """A decoded device map as the array functions take it: uint8 as it is, the uint16 bits of an int16 map as int32."""
    import torch
    return labels if labels.dtype == torch.uint8 else labels.to(torch.int32) & 0xffff


def labels_for_writer(rw, seg, properties: dict, compress_on_device: bool = False):
    """A device label map -> what ``rw.write_seg`` takes on a thread that makes no GPU call: the map on the host in its
    file's frame, or with ``compress_on_device`` the ``DeviceCompressedLabels`` of ``rw.compress_labels``."""
    import torch
    if seg.dtype not in (torch.uint8, torch.int16):
        seg = seg.to(torch.uint8) if seg.numel() == 0 or int(seg.max()) < 255 else seg.to(torch.int16)
    if compress_on_device:
        return rw.compress_labels(seg, properties)
    if hasattr(rw, 'labels_to_file_frame'):
        return rw.labels_to_file_frame(seg, properties)
    host = seg.cpu().numpy()
    return host.view('uint16') if host.dtype.itemsize == 2 else host
