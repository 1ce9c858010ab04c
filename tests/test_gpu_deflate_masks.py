"""The per-label mask encoder on a real MI355X: ``fnn_deflate_masks_count`` / ``fnn_deflate_masks_emit`` against the Python
model of the mask fragment (tests/deflate_masks_ref.py) byte for byte, zlib's inflate and ``zlib.crc32``; and ``JHUPredictor``
with ``compress_on_device`` against its default route and against ``nnUNetPredictor``'s label file.

Kernels launched here (csrc/deflate_masks.hip): deflate_masks_count_kernel<1> / <2>, deflate_masks_scan_kernel,
deflate_masks_emit_kernel<1> / <2> - ``test_every_kernel_is_launched`` reads their names from ``fnn_op_last_kernels``.
Lengths lie around the chunk (C = 16 KiB of mask bytes, one workgroup); ``out`` starts at an odd address between canaries
and ``work`` has exactly the stated size with canaries behind it.
"""
import gzip
import os
import threading
import zlib

import numpy as np
import pytest
import torch

import deflate_masks_ref as masks_ref
import deflate_ref
import nifti_ref
from test_gpu_deflate import _edge_runs
from test_gpu_predictor import _toy_model_folder
from test_gpu_reorient import PATCH, TRANSPOSE_ORIENTATION, _oriented_file, _small_ras

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda', 0)
C = deflate_ref.CHUNK
LENGTHS = (1, 255, C - 1, C, C + 1, 3 * C + 5, 40 * C + 123)        # elements
FRONT, BACK, FILL = 67, 64, 0xA5                                  # canary bytes around `out` (an odd address), their value
# labels with a part to play (a 2-byte map holds them with 0x0300 added, next to 1, 257 and 513: equal low bytes)
SOME, FIRST, LAST, TAIL, ABSENT = 21, 22, 23, 24, 25


def _label_map(n, wide):
    """n labels: runs that cross segment and chunk edges (``_edge_runs``), label 0 as background (1 in a 2-byte map, which
    holds 0 in a short run), SOME in the chunks 1 and 3 only, FIRST only as the first byte of a chunk, LAST only as the last
    byte of one, TAIL only in the last partial chunk; ABSENT nowhere."""
    a = _edge_runs(n)
    up = 0x0300 if wide else 0
    if wide:
        a = np.where(a == 0, 1, np.where(a >= 150, 257, 513))
        a[7:10] = 0
    for chunk in (1, 3):
        a[chunk * C + 500:chunk * C + 1500:3] = SOME + up           # (single voxels, and none where n is too short)
        a[chunk * C + 2000:chunk * C + 2300] = SOME + up
    if n < C:
        a[:1] = FIRST + up
        if n > 1:
            a[n - 1] = LAST + up
    else:
        a[(n // C // 2) * C] = FIRST + up
        a[(n // C // 2 + 1) * C - 1] = LAST + up
        if n % C > 2:
            a[n - n % C + 1:n - 1] = TAIL + up
    return a[:n].astype(np.uint16 if wide else np.uint8)


def _label_lists(wide):
    """Unsorted lists of 1, 3, 33 (crosses a 32-bit presence word) and 65 (more than a wave) labels, and 300 on a 2-byte map:
    the labels with a part, a few of the map's run values, and values that occur nowhere."""
    up = 0x0300 if wide else 0
    core = [LAST + up, 0, FIRST + up, ABSENT + up, SOME + up, TAIL + up] + ([257, 513, 1, 2] if wide else [300, 153, 33])
    filler = [v for v in np.random.default_rng(33).permutation(np.arange(1000, 60000, 7) if wide else np.arange(40, 150)).tolist()]
    return [[SOME + up], core[:3], core + filler[:33 - len(core)], filler[:20] + core[::-1] + filler[20:65 - len(core)]] \
        + ([filler[:150] + core + filler[150:300 - len(core)]] if wide else [])


_REFERENCE = {}


def _reference(n, wide, label):
    """(fragment, mask bytes) of the model, computed once per (map, label)."""
    key = (n, wide, label)
    if key not in _REFERENCE:
        seg = _label_map(n, wide)
        _REFERENCE[key] = (masks_ref.mask_fragment(seg, label), masks_ref.mask_of(seg, label).tobytes())
    return _REFERENCE[key]


def _encode(seg, labels, front=FRONT):
    """-> (sizes, crcs, fragments) of one count + emit, with every check that needs the device buffers."""
    from fast_nnunet_amd import capi
    size, n = seg.dtype.itemsize, seg.size
    stream = torch.cuda.current_stream(DEV).cuda_stream
    src = torch.from_numpy(seg.view(np.uint8).copy()).to(DEV) if n else torch.zeros(16, dtype=torch.uint8, device=DEV)
    assert src.data_ptr() % 16 == 0
    work_cap = capi.deflate_masks_work_bytes(n, len(labels))
    assert work_cap == masks_ref.work_bytes(n, len(labels))
    work = torch.full((work_cap + BACK,), FILL, dtype=torch.uint8, device=DEV)
    sizes, crcs = capi.deflate_masks_count(src.data_ptr(), size, n, labels, work.data_ptr(), work_cap, stream)
    assert capi.op_last_kernels() == ([f'deflate_masks_count_kernel<{size}>', 'deflate_masks_scan_kernel'] if n else [])
    assert bool((work[work_cap:] == FILL).all()), 'count wrote behind work'
    total = sum(sizes)
    buf = torch.full((front + total + BACK,), FILL, dtype=torch.uint8, device=DEV)
    capi.deflate_masks_emit(src.data_ptr(), size, n, labels, work.data_ptr(), buf.data_ptr() + front, total, stream)
    assert capi.op_last_kernels() == ([f'deflate_masks_emit_kernel<{size}>'] if n else [])
    host = buf.cpu().numpy()
    assert np.all(host[:front] == FILL) and np.all(host[front + total:] == FILL), 'wrote outside out[0, sum of the sizes)'
    assert bool((work[work_cap:] == FILL).all())
    assert np.array_equal(src.cpu().numpy()[:n * size], seg.view(np.uint8)), 'the input is left alone'
    ends = np.cumsum([0] + sizes) + front
    return sizes, crcs, [host[ends[k]:ends[k + 1]].tobytes() for k in range(len(labels))]


def _check(n, wide, labels, **kw):
    seg = _label_map(n, wide)
    sizes, crcs, frags = _encode(seg, labels, **kw)
    for label, nb, crc, frag in zip(labels, sizes, crcs, frags):
        where = f'{n} elements of {seg.dtype}, label {label} of {len(labels)}'
        want, mask = _reference(n, wide, label)
        assert nb == len(want) == len(frag), f'{where}: {nb} bytes, the model gives {len(want)}'
        if frag != want:
            i = next(k for k in range(len(want)) if frag[k] != want[k])
            raise AssertionError(f'{where}: first difference from the model at byte {i} of {len(want)}')
        d = zlib.decompressobj(-15)
        plain = d.decompress(frag + b'\x03\x00') + d.flush()
        assert d.eof and d.unused_data == b'' and plain == mask, f'{where}: inflate does not return the mask'
        assert crc == zlib.crc32(mask), where
    return frags


@pytest.mark.parametrize('wide', (False, True), ids=('uint8', 'uint16'))
@pytest.mark.parametrize('n', LENGTHS)
def test_fragments_equal_the_model_and_inflate_to_the_masks(n, wide):
    seg = _label_map(n, wide)
    up = 0x0300 if wide else 0
    present = set(np.unique(seg).tolist())
    assert ABSENT + up not in present and (0 in present or n < 10) and (not wide or n < 3 * C or {1, 257, 513} <= present)
    if n > 3 * C:
        assert {SOME + up, FIRST + up, LAST + up, TAIL + up} <= present
        assert (seg == FIRST + up).sum() == 1 and np.flatnonzero(seg == FIRST + up)[0] % C == 0
        assert (seg == LAST + up).sum() == 1 and np.flatnonzero(seg == LAST + up)[0] % C == C - 1
        assert np.flatnonzero(seg == TAIL + up).min() >= n - n % C
        assert set(np.flatnonzero(seg == SOME + up) // C) == ({1, 3} if n > 4 * C else {1}), 'absent from most chunks'
    for labels in _label_lists(wide):
        first = _check(n, wide, labels)
        if len(labels) == 33 and n in (1, C + 1, LENGTHS[-1]):
            assert _encode(seg, labels)[2] == first, f'{n} elements: two runs differ'
            assert _encode(seg, labels, front=64)[2] == first, f'{n} elements: the bytes depend on where out lies'


def test_golden_mask(golden_dir):
    voxels = np.frombuffer(gzip.decompress(open(os.path.join(golden_dir, 'example_ct_sm_T300_output.nii.gz'), 'rb').read())[352:], np.uint8)
    labels = sorted(set(np.unique(voxels).tolist()) | {200})[::-1]
    for seg in (voxels, voxels.astype(np.uint16)):
        sizes, crcs, frags = _encode(seg, labels)
        for label, crc, frag in zip(labels, crcs, frags):
            assert frag == masks_ref.mask_fragment(voxels, label) and crc == zlib.crc32(masks_ref.mask_of(voxels, label).tobytes())
            assert deflate_ref.inflate(frag) == masks_ref.mask_of(voxels, label).tobytes()


def test_refused_calls_return_their_codes_and_launch_nothing():
    from fast_nnunet_amd import capi
    n, OUT = C + 64, 1 << 15
    a = (torch.arange(n, device=DEV) % 7).to(torch.uint8)
    keep = a.clone()
    labels = [3, 1, 300]
    work_cap = capi.deflate_masks_work_bytes(n, 3)
    work = torch.full((work_cap + 16,), FILL, dtype=torch.uint8, device=DEV)
    out = torch.full((OUT,), FILL, dtype=torch.uint8, device=DEV)
    host = np.zeros(work_cap + 64, np.uint8)
    host_ptr = host.ctypes.data - host.ctypes.data % 16 + 16

    def count(in_ptr=None, size=1, n=n, labels=labels, work_ptr=None, cap=work_cap):
        return capi.deflate_masks_count(a.data_ptr() if in_ptr is None else in_ptr, size, n, labels,
                                        work.data_ptr() if work_ptr is None else work_ptr, cap)

    def emit(in_ptr=None, size=1, n=n, labels=labels, work_ptr=None, out_ptr=None, cap=OUT):
        return capi.deflate_masks_emit(a.data_ptr() if in_ptr is None else in_ptr, size, n, labels,
                                       work.data_ptr() if work_ptr is None else work_ptr,
                                       out.data_ptr() if out_ptr is None else out_ptr, cap)

    common = (('NULL', dict(in_ptr=0), AssertionError), ('NULL', dict(work_ptr=0), AssertionError),
              ('device', dict(in_ptr=host_ptr), AssertionError), ('device', dict(work_ptr=host_ptr), AssertionError),
              ('aligned', dict(in_ptr=a.data_ptr() + 8), AssertionError), ('aligned', dict(in_ptr=a.data_ptr() + 2, size=2, n=16), AssertionError),
              ('aligned', dict(work_ptr=work.data_ptr() + 8), AssertionError),
              ('1 or 2', dict(size=0), AssertionError), ('1 or 2', dict(size=3), AssertionError), ('1 or 2', dict(size=4, n=16), AssertionError),
              ('negative', dict(n=-1), AssertionError), ('at least 1', dict(labels=[]), AssertionError),
              ('outside', dict(labels=[1, -1]), AssertionError), ('outside', dict(labels=[65536]), AssertionError),
              ('twice', dict(labels=[4, 1, 4]), AssertionError),
              ('too many', dict(n=2 ** 45 + 1), NotImplementedError), ('too many', dict(n=2 ** 46, size=2), NotImplementedError))
    for match, kw, exc in common + (('work_cap', dict(cap=work_cap - 1), AssertionError), ('work_cap', dict(cap=0), AssertionError)):
        with pytest.raises(exc, match=match):
            count(**kw)
        assert capi.op_last_kernels() == [], (kw, 'a refused count launches nothing')
    sizes, crcs = count()
    assert capi.op_last_kernels() == ['deflate_masks_count_kernel<1>', 'deflate_masks_scan_kernel']
    total = sum(sizes)
    assert 0 < total <= OUT and sizes[2] == 112 + len(deflate_ref.chunk_bytes(bytes(64), 1)), 'label 300 on a 1-byte map: zeros'
    for match, kw, exc in common + (('NULL', dict(out_ptr=0), AssertionError), ('device', dict(out_ptr=host_ptr), AssertionError),
                                    ('out_cap', dict(cap=total - 1), AssertionError), ('out_cap', dict(cap=0), AssertionError),
                                    ('out_cap', dict(cap=-5), AssertionError), ('these labels', dict(labels=[3, 1, 2]), AssertionError)):
        with pytest.raises(exc, match=match):
            emit(**kw)
        assert capi.op_last_kernels() == [], (kw, 'a refused emit launches nothing')
    torch.cuda.synchronize()
    assert bool((out == FILL).all()) and bool((work[work_cap:] == FILL).all()) and bool((a == keep).all())
    # no elements: zero sizes, CRC 0, nothing launched, by either call
    assert count(n=0) == ([0, 0, 0], [0, 0, 0]) and capi.op_last_kernels() == []
    assert emit(n=0, cap=0) is None and capi.op_last_kernels() == []
    assert count(n=0, size=2, labels=[9]) == ([0], [0])
    # the limit is the chunk count, not 2^31 bytes: count and emit go through after all that
    sizes2, crcs2 = count()
    assert (sizes2, crcs2) == (sizes, crcs)
    emit(cap=total)
    assert capi.op_last_kernels() == ['deflate_masks_emit_kernel<1>']
    got = out.cpu().numpy()
    assert np.all(got[total:] == FILL)
    mask = (keep.cpu().numpy() == 3).astype(np.uint8).tobytes()
    assert deflate_ref.inflate(got[:sizes[0]].tobytes()) == mask and crcs[0] == zlib.crc32(mask)


def test_every_kernel_is_launched():
    """Every instantiation csrc/deflate_masks.hip holds, by the name ``fnn_op_last_kernels`` reports (``_encode`` asserts the
    names of each call against the element size)."""
    from fast_nnunet_amd import capi
    stream = torch.cuda.current_stream(DEV).cuda_stream
    seen = set()
    for dtype in (np.uint8, np.uint16):
        seg = (np.arange(C + 300) // 500).astype(dtype)
        src = torch.from_numpy(seg.view(np.uint8).copy()).to(DEV)
        work_cap = capi.deflate_masks_work_bytes(seg.size, 2)
        work = torch.empty(work_cap, dtype=torch.uint8, device=DEV)
        sizes, _ = capi.deflate_masks_count(src.data_ptr(), seg.dtype.itemsize, seg.size, [2, 40], work.data_ptr(), work_cap, stream)
        seen.update(capi.op_last_kernels())
        out = torch.empty(sum(sizes), dtype=torch.uint8, device=DEV)
        capi.deflate_masks_emit(src.data_ptr(), seg.dtype.itemsize, seg.size, [2, 40], work.data_ptr(), out.data_ptr(), sum(sizes), stream)
        seen.update(capi.op_last_kernels())
        assert out[:sizes[0]].cpu().numpy().tobytes() == masks_ref.mask_fragment(seg, 2)
    assert seen == {'deflate_masks_count_kernel<1>', 'deflate_masks_count_kernel<2>', 'deflate_masks_scan_kernel',
                    'deflate_masks_emit_kernel<1>', 'deflate_masks_emit_kernel<2>'}


# ---------------------------------------------------------------------------------------------------------------
# the reader-writers and the case pipeline
# ---------------------------------------------------------------------------------------------------------------
def _predictors(tmp, name):
    """The toy model folder of tests/test_gpu_predictor.py read by nnUNetPredictor and by two JHUPredictors: the default and
    compress_on_device."""
    import json
    from fast_nnunet_amd import nnUNetPredictor
    from fast_nnunet_amd.jhu import JHUPredictor
    folder, plans, dj, sd, spec = _toy_model_folder(tmp, PATCH, 3, plans_spacing=(3.0, 3.0, 3.0))
    if name is not None:
        (folder / 'dataset.json').write_text(json.dumps(dict(dj, overwrite_image_reader_writer=name)))
    made = []
    for cls, flag in ((nnUNetPredictor, False), (JHUPredictor, False), (JHUPredictor, True)):
        p = cls(tile_step_size=0.5, use_gaussian=True, use_mirroring=False, device=DEV, allow_tqdm=False,
                patches_per_forward=4, compress_on_device=flag)
        p.initialize_from_trained_model_folder(str(folder), use_folds=(0,))
        made.append(p)
    return made


def _files_under(folder):
    return sorted(os.path.relpath(os.path.join(d, f), folder) for d, _, fs in os.walk(folder) for f in fs)


@pytest.mark.parametrize('name', (None, 'NibabelIOWithReorient'), ids=('NiftiIO', 'NibabelIOWithReorient'))
def test_jhu_predictor_writes_the_same_mask_files_on_both_routes(tmp_path, name):
    from fast_nnunet_amd.imageio import DeviceCompressedLabels, NiftiIO, NiftiReorientIO
    plain, default, device = _predictors(tmp_path, name)
    assert type(device._reader_writer()) is (NiftiIO if name is None else NiftiReorientIO) and device.compress_on_device
    src = tmp_path / 'in'
    src.mkdir()
    perm, signs = TRANSPOSE_ORIENTATION
    n = 2
    for i in range(n):
        _oriented_file(str(src / f'c{i}_0000.nii.gz'), _small_ras(70 + i), 4, perm, signs)
    out = {k: tmp_path / k for k in ('plain', 'default', 'threads', 'sequential')}
    assert plain.predict_from_files(str(src), str(out['plain'])) == [None] * n
    assert default.predict_from_files(str(src), str(out['default'])) == [None] * n
    assert device.predict_from_files(str(src), str(out['threads']), num_processes_preprocessing=2,
                                     num_processes_segmentation_export=2) == [None] * n
    assert device.predict_from_files_sequential(str(src), str(out['sequential'])) == [None] * n
    masks = [os.path.join(f'c{i}', 'predictions', f'c{l}.nii.gz') for i in range(n) for l in (1, 2)]
    run_files = ['dataset.json', 'plans.json', 'predict_from_raw_data_args.json']
    for k in ('default', 'threads', 'sequential'):
        assert _files_under(out[k]) == sorted(masks + run_files), f'{k}: one mask per foreground label and no label file'
    classes = set()
    for i in range(n):
        labels, info = nifti_ref.read(str(out['plain'] / f'c{i}.nii.gz'))
        header = gzip.decompress(open(out['plain'] / f'c{i}.nii.gz', 'rb').read())[:352]             # (a uint8 file too)
        classes.update(np.unique(labels).tolist())
        for l in (1, 2):
            rel = os.path.join(f'c{i}', 'predictions', f'c{l}.nii.gz')
            a = open(out['default'] / rel, 'rb').read()
            host_mask = (np.asarray(labels) == l).astype(np.uint8)
            for k in ('threads', 'sequential'):
                b = open(out[k] / rel, 'rb').read()
                assert gzip.decompress(a) == gzip.decompress(b), f'{k}/{rel}: other header or voxels'
                assert a != b and a[:10] == b[:10], f'{k}/{rel}: the device route was not taken'
            assert open(out['threads'] / rel, 'rb').read() == open(out['sequential'] / rel, 'rb').read()
            got, got_info = nifti_ref.read(str(out['threads'] / rel))
            assert np.array_equal(got, host_mask), f'{rel}: not (labels == {l}) of the label file'
            assert np.array_equal(got_info['sform'], info['sform'])
            # the default route's file: the label file's header in front of the mask's bytes, through the same writer
            assert gzip.decompress(a) == header + host_mask.tobytes(), f'default/{rel}'
    assert len(classes) >= 2, 'label maps with more than background'
    # one array with an output target and probabilities: the folder, and .npz / .pkl next to it; no target: nnUNetPredictor's result
    rw = device._reader_writer()
    img, props = rw.read_images([str(src / 'c0_0000.nii.gz')], on_device=False)
    for p, k in ((device, 'single'), (default, 'single_default')):
        assert p.predict_single_npy_array(img, props, output_file_truncated=str(tmp_path / k), save_or_return_probabilities=True) is None
        assert sorted(os.listdir(tmp_path / k / 'predictions')) == ['c1.nii.gz', 'c2.nii.gz'] and not os.path.exists(tmp_path / f'{k}.nii.gz')
    assert open(tmp_path / 'single' / 'predictions' / 'c1.nii.gz', 'rb').read() == open(out['threads'] / 'c0' / 'predictions' / 'c1.nii.gz', 'rb').read()
    assert open(tmp_path / 'single_default' / 'predictions' / 'c2.nii.gz', 'rb').read() == open(out['default'] / 'c0' / 'predictions' / 'c2.nii.gz', 'rb').read()
    assert np.array_equal(np.load(tmp_path / 'single.npz')['probabilities'], np.load(tmp_path / 'single_default.npz')['probabilities'])
    assert open(tmp_path / 'single.pkl', 'rb').read() == open(tmp_path / 'single_default.pkl', 'rb').read()
    seg = device.predict_single_npy_array(img, props)
    assert isinstance(seg, np.ndarray) and np.array_equal(seg, plain.predict_single_npy_array(img, props))
    # the reader-writer's own method: a device map in, one value per label out, in the order asked for
    made = rw.compress_label_masks(torch.from_numpy(seg).to(DEV), [2, 1, 9], props)
    assert len(made) == 3 and all(isinstance(m, DeviceCompressedLabels) and not m.uint16 and m.n_bytes == seg.size for m in made)
    rw.write_seg(made[1], str(tmp_path / 'own.nii.gz'), props)
    assert open(tmp_path / 'own.nii.gz', 'rb').read() == open(out['threads'] / 'c0' / 'predictions' / 'c1.nii.gz', 'rb').read()
    assert deflate_ref.inflate(made[2].fragment) == bytes(seg.size) and made[2].crc32 == zlib.crc32(bytes(seg.size))
    assert rw.compress_label_masks(torch.from_numpy(seg).to(DEV), [], props) == []
    with pytest.raises(TypeError, match='GPU'):
        rw.compress_label_masks(seg, [1], props)
    assert not [t.name for t in threading.enumerate() if t.name.startswith('fnn-')], 'reader and writer threads have ended'
    left = [f for d, _, fs in os.walk(tmp_path) for f in fs if '.part' in f]
    assert not left, left
