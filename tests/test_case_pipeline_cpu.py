"""``case_pipeline`` without a GPU: the order in which ``run_pipeline`` stages, reads, runs and exports fake cases on its
threads (every order is forced or observed with Events and one recorded event list: nothing sleeps), what a failing case
leaves behind, the atomic case writer, and ``labels_for_writer`` on CPU tensors through ``write_seg`` into files that
tests/nifti_ref.py reads back."""
import os
import threading

import numpy as np
import pytest
import torch

import nifti_ref
import orient_ref as oref

WAIT = 60                                                        # seconds an Event may take before a test fails (never reached)
FLAGS = [(True, True), (True, False), (False, True), (False, False)]
FLAG_IDS = ['reader+writer', 'reader', 'writer', 'inline']


class Cases:
    """``stage`` and ``run`` of fake cases that record (what, i, thread name).  With a writer thread export i is held until
    ``run(i + 1)`` has ended, and with a reader thread ``run(i)`` ends only once fill i + 1 has begun."""

    def __init__(self, n, read_thread, write_thread, fail=None):
        self.n, self.read_thread, self.write_thread, self.fail = n, read_thread, write_thread, fail
        self.events, self.lock = [], threading.Lock()
        self.fill_begun = [threading.Event() for _ in range(n)]
        self.export_begun = [threading.Event() for _ in range(n)]
        self.release = [threading.Event() for _ in range(n)]

    def say(self, what, i):
        with self.lock:
            self.events.append((what, i, threading.current_thread().name))

    def boom(self, what, i):
        if self.fail == (what, i):
            raise Boom(f'{what} {i} failed')

    def stage(self, i):
        self.say('stage', i)

        def fill():
            self.say('fill_begin', i)
            self.fill_begun[i].set()
            self.boom('fill', i)
            self.say('fill_end', i)
            return 10 * i
        return fill

    def run(self, i, data):
        self.say('run_begin', i)
        assert data == 10 * i
        self.boom('run', i)
        if self.read_thread and i + 1 < self.n:
            assert self.fill_begun[i + 1].wait(WAIT), 'case i + 1 is read while case i runs'
        if self.write_thread and i > 0 and self.fail is None:
            assert self.export_begun[i - 1].wait(WAIT), 'export i - 1 is under way while case i runs'
        self.say('run_end', i)
        if i > 0:
            self.release[i - 1].set()

        def export():
            self.say('export_begin', i)
            self.export_begun[i].set()
            self.boom('export', i)
            if self.write_thread and i + 1 < self.n and self.fail is None:
                assert self.release[i].wait(WAIT)
            self.say('export_end', i)
        return ('result', i), export

    def at(self, what, i):
        return [(w, k) for w, k, _ in self.events].index((what, i))

    def threads(self, what):
        return {t for w, _, t in self.events if w.startswith(what)}

    def done(self, what):
        return [k for w, k, _ in self.events if w == what]


class Boom(Exception):
    pass


def _no_pipeline_thread():
    return not [t.name for t in threading.enumerate() if t.name.startswith('fnn-')]


@pytest.mark.parametrize('read_thread, write_thread', FLAGS, ids=FLAG_IDS)
def test_loop_order(read_thread, write_thread):
    from fast_nnunet_amd.case_pipeline import run_pipeline
    n, me = 5, threading.current_thread().name
    c = Cases(n, read_thread, write_thread)
    results = run_pipeline(n, c.stage, c.run, read_thread=read_thread, write_thread=write_thread)
    assert results == [('result', i) for i in range(n)], 'in case order, the same for every combination'
    assert _no_pipeline_thread()
    assert c.threads('stage') == {me} and c.threads('run') == {me}
    assert c.threads('fill') == {'fnn-reader' if read_thread else me}
    assert c.threads('export') == {'fnn-writer' if write_thread else me}
    for what in ('stage', 'fill_begin', 'fill_end', 'run_begin', 'run_end', 'export_begin', 'export_end'):
        assert c.done(what) == list(range(n)), what
    for i in range(n):
        assert c.at('stage', i) < c.at('fill_begin', i) and c.at('fill_end', i) < c.at('run_begin', i)
        assert c.at('run_end', i) < c.at('export_begin', i)
        if i + 1 < n:
            assert c.at('stage', i + 1) < c.at('run_begin', i), 'fill i + 1 was handed over before run(i) started'
            if not read_thread:
                assert c.at('fill_end', i + 1) < c.at('run_begin', i), 'inline: read where it would have been handed over'
        if i > 0:
            assert c.at('export_end', i - 1) < c.at('export_begin', i), 'at most one case waits for the disk'
            if write_thread:
                # export i - 1 was held until run(i) had ended: the case ran while the one before it was being written
                assert c.at('export_begin', i - 1) < c.at('run_end', i) < c.at('export_end', i - 1)
            else:
                assert c.at('export_end', i - 1) < c.at('run_begin', i), 'inline: written before the next case runs'


def test_results_without_exports_and_no_case_starts_no_thread(monkeypatch):
    from fast_nnunet_amd import case_pipeline
    got = case_pipeline.run_pipeline(3, lambda i: (lambda: i), lambda i, data: ((i, data), None), write_thread=True)
    assert got == [(0, 0), (1, 1), (2, 2)] and _no_pipeline_thread()

    def refuse(*a, **k):
        raise AssertionError('no case: nothing to start or to call')
    monkeypatch.setattr(case_pipeline, 'HostWorker', refuse)
    for read_thread, write_thread in FLAGS:
        assert case_pipeline.run_pipeline(0, refuse, refuse, read_thread=read_thread, write_thread=write_thread) == []


@pytest.mark.parametrize('threads', [True, False], ids=['threads', 'inline'])
@pytest.mark.parametrize('fail', [('fill', 1), ('run', 1), ('export', 0)], ids=['fill1', 'run1', 'export0'])
def test_a_failure_surfaces_in_the_calling_thread_and_ends_the_threads(fail, threads):
    from fast_nnunet_amd.case_pipeline import run_pipeline
    c = Cases(3, threads, threads, fail=fail)
    with pytest.raises(Boom) as e:
        run_pipeline(3, c.stage, c.run, read_thread=threads, write_thread=threads)
    assert type(e.value) is Boom and str(e.value) == f'{fail[0]} {fail[1]} failed'
    assert _no_pipeline_thread()
    # with threads a failure is met where its job is waited for; inline it is raised where it happens
    ran = {(('fill', 1), True): [0], (('fill', 1), False): [], (('run', 1), True): [0, 1], (('run', 1), False): [0, 1],
           (('export', 0), True): [0, 1], (('export', 0), False): [0]}[(fail, threads)]
    assert c.done('run_begin') == ran, 'run is never called for a later case'
    begun = [i for i in c.done('export_begin') if ('export', i) != fail]
    assert c.done('export_end') == begun, 'an export handed over before the failure has completed'
    assert begun == ([] if fail == ('export', 0) or (fail == ('fill', 1) and not threads) else [0])


# ---------------------------------------------------------------------------------------------------------------
# the case writer
# ---------------------------------------------------------------------------------------------------------------
PROBS = np.zeros((2, 3, 4, 5), np.float32)
PROPS = {'spacing': [1.0, 1.0, 1.0], 'shape_before_cropping': (3, 4, 5)}


def test_case_writer_leaves_the_case_files_and_what_the_label_callback_made(tmp_path):
    from fast_nnunet_amd.case_pipeline import export_case_files
    from fast_nnunet_amd.ensembling import load_properties_pkl
    trunc = os.path.join(tmp_path, 'case')
    export_case_files(trunc, PROBS, PROPS, lambda: open(trunc + '.nii.gz', 'wb').close())
    assert sorted(os.listdir(tmp_path)) == ['case.nii.gz', 'case.npz', 'case.pkl']
    assert np.array_equal(np.load(trunc + '.npz')['probabilities'], PROBS) and load_properties_pkl(trunc + '.pkl') == PROPS
    other = os.path.join(tmp_path, 'other')
    export_case_files(other, None, PROPS, lambda: open(other + '.nii.gz', 'wb').close())
    assert sorted(os.listdir(tmp_path)) == ['case.nii.gz', 'case.npz', 'case.pkl', 'other.nii.gz']


def test_case_writer_with_properties_that_cannot_be_pickled(tmp_path):
    from fast_nnunet_amd.case_pipeline import export_case_files
    called = []
    with pytest.raises(Exception, match='pickle'):
        export_case_files(os.path.join(tmp_path, 'case'), PROBS, {'spacing': lambda: 1}, lambda: called.append(1))
    assert os.listdir(tmp_path) == ['case.npz'] and not called, 'no .pkl, no .part*, no label file'


def test_case_writer_with_a_raising_label_callback(tmp_path):
    from fast_nnunet_amd.case_pipeline import export_case_files

    def write_labels():
        raise Boom('no label file')
    with pytest.raises(Boom, match='no label file'):
        export_case_files(os.path.join(tmp_path, 'case'), PROBS, PROPS, write_labels)
    assert sorted(os.listdir(tmp_path)) == ['case.npz', 'case.pkl']


# ---------------------------------------------------------------------------------------------------------------
# the label hand-off
# ---------------------------------------------------------------------------------------------------------------
SHAPE = (3, 4, 5)
# (torch dtype, a label the map holds besides 0..200) -> the file's NIfTI datatype: uint8 (2) below 255, uint16 (512) from 255 on
HANDOFF = {'uint8_254': (torch.uint8, 254, 2), 'uint8_255': (torch.uint8, 255, 512), 'int32_300': (torch.int32, 300, 512),
           'int32_40000': (torch.int32, 40000, 512)}
PERM, SIGNS = (1, 0, 2), (1, -1, -1)                             # a flipped and permuted file frame


def _label_map(top):
    a = (np.arange(int(np.prod(SHAPE)), dtype=np.int64) * 37 % 201).reshape(SHAPE)
    a[1, 2, 3] = top
    return a


@pytest.mark.parametrize('reorient', [False, True], ids=['NiftiIO', 'NiftiReorientIO'])
@pytest.mark.parametrize('case', list(HANDOFF))
def test_label_handoff_writes_the_voxels_and_the_file_type(case, reorient, tmp_path):
    from fast_nnunet_amd import imageio
    from fast_nnunet_amd.case_pipeline import labels_for_writer
    dtype, top, datatype = HANDOFF[case]
    in_file = _label_map(top)                                    # (z, y, x) as the file holds it
    if reorient:
        rw = imageio.NiftiReorientIO()
        affine = oref.affine_of(PERM, SIGNS)
        o = imageio.Reorientation(affine, SHAPE[::-1])
        props = {'nibabel_stuff': {'original_affine': o.original_affine, 'reoriented_affine': o.reoriented_affine}}
        handed = oref.apply_zyx(in_file, oref.ornt_of(PERM, SIGNS))           # the RAS frame, by the tests' own rule
        assert handed.shape != in_file.shape
    else:
        rw = imageio.NiftiIO()
        affine = np.diag([1.5, 1.5, 2.0, 1.0])
        props = {'nibabel_stuff': {'original_affine': affine}}
        handed = in_file
    labels = torch.from_numpy(np.ascontiguousarray(handed)).to(dtype)
    out = labels_for_writer(rw, labels, props)
    assert isinstance(out, imageio.FileFrameLabels if reorient else np.ndarray)
    voxels = out.voxels if reorient else out
    assert voxels.dtype == (np.uint8 if dtype == torch.uint8 else np.uint16), 'two-byte voxels reach the writer as uint16'
    fname = os.path.join(tmp_path, 'labels.nii.gz')
    rw.write_seg(out, fname, props)
    values, info = nifti_ref.read(fname)
    assert int(info['header']['datatype']) == datatype
    assert values.shape == SHAPE and np.array_equal(values.astype(np.int64), in_file)
    assert np.array_equal(info['sform'].astype(np.float32), affine.astype(np.float32))
    # the caller's width gives the same file (a map narrower than its width is narrowed by the writer, as always)
    wide = labels_for_writer(rw, labels, props, u16=True)
    assert (wide.voxels if reorient else wide).dtype == np.uint16
    rw.write_seg(wide, fname + '.wide.nii.gz', props)
    assert open(fname + '.wide.nii.gz', 'rb').read() == open(fname, 'rb').read()


def test_labels_that_go_to_no_file_and_the_compress_predicate():
    from fast_nnunet_amd.case_pipeline import device_compressor, labels_for_writer
    from fast_nnunet_amd.imageio import NiftiIO, NiftiReorientIO
    labels = torch.from_numpy(_label_map(40000)).to(torch.int32)
    host = labels_for_writer(None, labels, None, u16=True)
    assert host.dtype == np.uint16 and np.array_equal(host, _label_map(40000))
    host = labels_for_writer(None, torch.from_numpy(_label_map(7)).to(torch.int32), None, u16=False)
    assert host.dtype == np.uint8 and np.array_equal(host, _label_map(7))
    made = []
    assert labels_for_writer(NiftiIO(), labels, {'p': 1}, compress=lambda seg, props: made.append((seg.dtype, props)) or 'made') == 'made'
    assert made == [(torch.int16, {'p': 1})]
    for rw in (NiftiIO(), NiftiReorientIO()):
        assert device_compressor(rw, True, '.nii.gz') == rw.compress_labels
        assert device_compressor(rw, True, '.NII.GZ', 'compress_label_masks') == rw.compress_label_masks
        assert device_compressor(rw, False, '.nii.gz') is None and device_compressor(rw, True, '.nii') is None
    assert device_compressor(object(), True, '.nii.gz') is None, 'a reader-writer that cannot compress'
