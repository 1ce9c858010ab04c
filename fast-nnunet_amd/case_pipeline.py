"""What every way from files to files shares: the reader / GPU / writer case loop, the atomic writer of a case's ``.npz`` and
``.pkl``, and the step from a label tensor to what a reader-writer's ``write_seg`` takes.

``nnUNetPredictor.predict_from_files``, ``label_folders.run_label_cases`` (evaluation, postprocessing) and
``ensembling.ensemble_folders`` are clients of ``run_pipeline``: the calling thread is the only one that touches the GPU, one
``HostWorker`` reads (and inflates) case i + 1 while case i runs, a second one writes case i - 1.  No process is started.
"""
from __future__ import annotations

import functools
import os
import pickle
import queue
import threading
from typing import Callable, Optional

import numpy as np
import torch


class Job:
    def __init__(self, fn):
        self.fn, self.done, self.value, self.error = fn, threading.Event(), None, None

    def run(self) -> 'Job':
        try:
            self.value = self.fn()
        except BaseException as e:                               # handed to the thread that waits for the job
            self.error = e
        self.done.set()
        return self

    def result(self):
        self.done.wait()
        if self.error is not None:
            raise self.error
        return self.value


class HostWorker:
    """One thread that runs host-only jobs (file reads, zlib, file writes) in order; it never makes a GPU call."""

    def __init__(self, name: str):
        self.q = queue.Queue()
        self.t = threading.Thread(target=self._run, name=name, daemon=True)
        self.t.start()

    def _run(self):
        for job in iter(self.q.get, None):
            job.run()

    def submit(self, fn) -> Job:
        job = Job(fn)
        self.q.put(job)
        return job

    def close(self):
        """Runs what is queued, then ends the thread."""
        self.q.put(None)
        self.t.join()


def run_pipeline(n_cases: int, stage: Callable, run: Callable, read_thread: bool = True, write_thread: bool = False) -> list:
    """The case loop of every file front-end.

    ``stage(i)`` runs on the calling thread (it may allocate pinned memory) and returns a host-only callable that reads case
    i - run on the reader thread ``fnn-reader``, its value handed to ``run``.  ``run(i, data)`` runs on the calling thread (the
    GPU part) and returns ``(result, export)``: ``export`` is None or a host-only callable that writes the case's files, run
    on the writer thread ``fnn-writer``.  Case i + 1 is read while case i runs, and at most one case waits for the disk.
    Without ``read_thread`` / ``write_thread`` that side runs on the calling thread, at the point where it would have been
    handed over.  Returns the results.  A failing case raises here, in the calling thread, after both threads have run what
    was handed to them and have been joined."""
    results = []
    if n_cases == 0:
        return results
    reader = HostWorker('fnn-reader') if read_thread else None
    writer = HostWorker('fnn-writer') if write_thread else None

    def hand(worker, fn) -> Job:
        if worker is not None:
            return worker.submit(fn)
        job = Job(fn).run()
        job.result()                                             # (inline: a failure is raised where it happens)
        return job

    try:
        nxt = hand(reader, stage(0))
        pending = None                                           # the writer's job for the previous case
        for i in range(n_cases):
            data = nxt.result()                                  # case i is in host memory (or its read failed)
            # case i + 1 is read while case i runs; its slot's buffers were released when case i - 1 was decoded
            nxt = hand(reader, stage(i + 1)) if i + 1 < n_cases else None
            result, export = run(i, data)
            results.append(result)
            if export is None:
                continue
            if pending is not None:
                pending.result()                                 # at most one case waits for the disk
            pending = hand(writer, export)
        if pending is not None:
            pending.result()
    finally:
        for w in (reader, writer):
            if w is not None:
                w.close()
    return results


def export_case_files(truncated: str, probabilities: Optional[np.ndarray], properties: dict, write_labels: Callable) -> None:
    """Host only (numpy, zlib, file writes): with probabilities ``<truncated>.npz`` and the properties as ``<truncated>.pkl``,
    each through a ``.part<pid>`` name and ``os.replace``, then ``write_labels()``, which makes the case's label file(s) the
    same way.  Every file appears under its name when it is complete and no ``.part`` file stays behind a failure."""
    made = []
    try:
        if probabilities is not None:
            for ending, dump in (('.npz', lambda f: np.savez_compressed(f, probabilities=probabilities)),
                                 ('.pkl', lambda f: pickle.dump(properties, f))):
                tmp = f'{truncated}{ending}.part{os.getpid()}'
                made.append(tmp)
                with open(tmp, 'wb') as f:
                    dump(f)
                os.replace(tmp, truncated + ending)
        write_labels()
    finally:
        for tmp in made:
            if os.path.exists(tmp):
                os.remove(tmp)


# ---- labels ------------------------------------------------------------------------------------------------------------
def as_plain_labels(labels: torch.Tensor) -> torch.Tensor:
    """A label map as the array functions take it: uint8 as it is, the uint16 bits of an int16 map as int32 (torch has no
    uint16 arithmetic)."""
    return labels if labels.dtype == torch.uint8 else labels.to(torch.int32) & 0xffff


def compress_mode(compress_on_device):
    """What the ``compress_on_device`` switch of the predictors and the folder commands accepts -> False, True (the fixed
    Huffman code of ``fnn_deflate_labels``) or ``'dynamic'`` (per-chunk tables, ``fnn_deflate_labels_dyn``); anything else
    is a ValueError."""
    if isinstance(compress_on_device, str):
        if compress_on_device == 'dynamic':
            return 'dynamic'
    elif isinstance(compress_on_device, (bool, int, np.bool_)) and compress_on_device in (0, 1):
        return bool(compress_on_device)
    raise ValueError(f"compress_on_device must be False, True or 'dynamic', got {compress_on_device!r}")


def device_compressor(rw, compress_on_device, file_ending: str, method: str = 'compress_labels'):
    """The reader-writer's ``method`` (``compress_labels`` or ``compress_label_masks``) when labels bound for a file of
    ``file_ending`` are to be compressed on the device and ``rw`` can; else None.  ``compress_on_device='dynamic'`` is
    ``compress_labels`` with ``tables='dynamic'``; the mask encoder has no dynamic tables (NotImplementedError)."""
    mode = compress_mode(compress_on_device)
    if mode == 'dynamic' and method != 'compress_labels':
        raise NotImplementedError(f"compress_on_device='dynamic': {method} (the per-label mask encoder, csrc/deflate_masks.hip) "
                                  "writes the fixed Huffman code only; use compress_on_device=True")
    if mode and str(file_ending).lower().endswith('.nii.gz'):
        fn = getattr(rw, method, None)
        if fn is not None and mode == 'dynamic':
            return functools.partial(fn, tables='dynamic')
        return fn
    return None


def labels_for_writer(rw, labels: torch.Tensor, properties: Optional[dict], u16: Optional[bool] = None,
                      compress: Optional[Callable] = None):
    """A label tensor (on the device or the CPU; uint8, the int16 that carries uint16 bits, or plain int32) -> what
    ``rw.write_seg`` takes on a thread that makes no GPU call.  ``u16`` is the width: the caller's rule, or None for the
    content rule (two bytes from a label of 255 on; a decoded uint8 / int16 map has its width already).  With ``compress``
    (``device_compressor``) its ``DeviceCompressedLabels``: the map is never downloaded; where ``rw`` reorients the
    ``FileFrameLabels`` of ``rw.labels_to_file_frame``; else (and with ``rw`` None: labels that go to no file) the host array.
    Two-byte voxels always reach the writer viewed as uint16."""
    if u16 is None:
        u16 = labels.dtype == torch.int16 or \
            (labels.dtype != torch.uint8 and labels.numel() > 0 and int(labels.max()) >= 255)
    labels = labels.to(torch.int16 if u16 else torch.uint8)     # (int16: the two bytes of the uint16 file type)
    if compress is not None:
        return compress(labels, properties)
    if hasattr(rw, 'labels_to_file_frame'):
        out = rw.labels_to_file_frame(labels, properties)
        out.voxels = out.voxels.view(np.uint16) if u16 else out.voxels
        return out
    host = labels.cpu().numpy()
    return host.view(np.uint16) if u16 else host
