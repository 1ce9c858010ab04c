"""The device deflate encoder on a real MI355X: ``fnn_deflate_labels`` against zlib's inflate, ``zlib.crc32`` and the Python
model of its token rule (tests/deflate_ref.py) byte for byte, and the case pipeline with ``compress_on_device=True`` against
the default route.

Kernels launched here (csrc/deflate.hip): deflate_max_kernel, deflate_count_kernel / deflate_emit_kernel <1,0> (uint8),
<2,0> (uint16) and <1,1> (a two-byte map written as uint8), deflate_scan_kernel - ``test_every_kernel_is_launched`` reads
their names from ``fnn_op_last_kernels``.  Lengths lie around the segment (S = 256 bytes, one lane) and the chunk
(C = 16 KiB, one wave); ``out`` starts at an odd address between canaries.
"""
import gzip
import os
import threading
import zlib

import numpy as np
import pytest
import torch

import deflate_ref
import nifti_ref
from test_gpu_predictor import _toy_model_folder
from test_gpu_reorient import PATCH, TRANSPOSE_ORIENTATION, _oriented_file, _small_ras

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda', 0)
S, C = deflate_ref.SEGMENT, deflate_ref.CHUNK
LENGTHS = (1, 2, 3, S - 1, S, S + 1, C - 1, C, C + 1, 2 * C + 1, 40 * C + 123)        # elements
FRONT, BACK, FILL = 67, 64, 0xA5                                  # canary bytes around `out` (an odd address), their value
MASK = 'example_ct_sm_T300_output.nii.gz'


def _runs(rng, n, lengths, values):
    """n values: runs whose lengths and values are drawn from the two sequences."""
    k = n // min(lengths) + 2
    return np.repeat(rng.choice(values, k), rng.choice(lengths, k))[:n]


def _edge_runs(n):
    """Runs that begin two bytes before and end one byte behind every segment and chunk edge, and values that change at it."""
    a = np.zeros(n, np.int64)
    for edge in range(S, n + S, S):
        a[max(edge - 2, 0):edge + 1] = 150 + (edge // S) % 90
        if edge % C == 0:
            a[max(edge - 300, 0):edge + 259] = 30 + (edge // C) % 100
    a[n // 2:] += 3
    return a


CONTENTS = {
    'constant': lambda rng, n: (np.full(n, 7, np.uint8), False),
    'runs_257_to_261': lambda rng, n: (_runs(rng, n, (257, 258, 259, 260, 261), np.arange(120, 170)).astype(np.uint8), False),
    'runs_over_edges': lambda rng, n: (_edge_runs(n).astype(np.uint8), False),
    'both_sides_of_144': lambda rng, n: (_runs(rng, n, (1, 2, 3, 4, 9), (143, 144, 0, 255, 145, 142)).astype(np.uint8), False),
    'random': lambda rng, n: (rng.integers(0, 256, n, dtype=np.uint8), False),
    'uint16_high_bytes': lambda rng, n: (_runs(rng, n, (1, 2, 3, 5, 40, 300), (0, 255, 256, 257, 1000, 65535, 0x9090)).astype(np.uint16), False),
    'uint16_random': lambda rng, n: (rng.integers(0, 65536, n, dtype=np.uint16), False),
    'uint16_narrows': lambda rng, n: (_runs(rng, n, (1, 2, 3, 7, 100), (0, 1, 2, 143, 144, 254)).astype(np.uint16), True),
    'uint16_stays_with_255': lambda rng, n: (np.append(_runs(rng, n - 1, (2, 50), (0, 3, 200)), 255).astype(np.uint16), True),
}


def _deflate(values, narrow, aligned_out=False):
    """-> (fragment bytes, bytes per element in the file, crc) of one call, with every check that needs the device buffer."""
    from fast_nnunet_amd import capi
    size = values.dtype.itemsize
    src = torch.from_numpy(values.view(np.uint8).copy()).to(DEV) if values.size else torch.zeros(16, dtype=torch.uint8, device=DEV)
    assert src.data_ptr() % 16 == 0
    cap = capi.deflate_bound(values.size * size)
    front = 64 if aligned_out else FRONT
    buf = torch.full((front + cap + BACK,), FILL, dtype=torch.uint8, device=DEV)
    n_out, file_size, crc = capi.deflate_labels(src.data_ptr(), size, values.size, narrow, buf.data_ptr() + front, cap,
                                                torch.cuda.current_stream(DEV).cuda_stream)
    want = [f'deflate_count_kernel<{file_size},{int(file_size != size)}>', 'deflate_scan_kernel',
            f'deflate_emit_kernel<{file_size},{int(file_size != size)}>'] if values.size else []
    assert capi.op_last_kernels() == (['deflate_max_kernel'] if narrow and size == 2 and values.size else []) + want
    host = buf.cpu().numpy()
    assert 0 <= n_out <= cap, f'{n_out} bytes, the bound is {cap}'
    assert np.all(host[:front] == FILL) and np.all(host[front + n_out:] == FILL), 'wrote outside out[0, out_bytes)'
    assert np.array_equal(src.cpu().numpy()[:values.size * size], values.view(np.uint8)), 'the input is left alone'
    return host[front:front + n_out].tobytes(), file_size, crc


def _file_bytes(values, narrow):
    if narrow and values.dtype.itemsize == 2 and (values.size == 0 or values.max() < 255):
        return values.astype(np.uint8).tobytes(), 1
    return values.astype(values.dtype.newbyteorder('<')).tobytes(), values.dtype.itemsize


def _check(values, narrow, where, **kw):
    frag, file_size, crc = _deflate(values, narrow, **kw)
    raw, want_size = _file_bytes(values, narrow)
    assert file_size == want_size, where
    d = zlib.decompressobj(-15)
    plain = d.decompress(frag + b'\x03\x00') + d.flush()
    assert d.eof and d.unused_data == b'' and plain == raw, f'{where}: inflate does not return the input'
    assert crc == zlib.crc32(raw), where
    want = deflate_ref.fragment(raw, file_size)
    if frag != want:
        i = next((k for k in range(min(len(frag), len(want))) if frag[k] != want[k]), min(len(frag), len(want)))
        raise AssertionError(f'{where}: {len(frag)} bytes, the model gives {len(want)}; first difference at byte {i}')
    return frag


@pytest.mark.parametrize('kind', list(CONTENTS))
def test_fragment_inflates_to_the_input_and_equals_the_model(kind):
    rng = np.random.default_rng(sorted(CONTENTS).index(kind))
    for n in LENGTHS:
        if kind == 'uint16_stays_with_255' and n < 2:
            continue
        values, narrow = CONTENTS[kind](rng, n)
        assert values.size == n
        first = _check(values, narrow, f'{kind}, {n} elements')
        if n in (3, C + 1, LENGTHS[-1]):
            again, _, _ = _deflate(values, narrow)
            assert again == first, f'{kind}, {n} elements: two runs differ'
            aligned, _, _ = _deflate(values, narrow, aligned_out=True)
            assert aligned == first, f'{kind}, {n} elements: the bytes depend on where out lies'


def test_golden_mask_and_the_size_condition(golden_dir):
    voxels = np.frombuffer(gzip.decompress(open(os.path.join(golden_dir, MASK), 'rb').read())[352:], np.uint8)
    for values, narrow in ((voxels, False), (voxels.astype(np.uint16), False), (voxels.astype(np.uint16), True)):
        frag = _check(values, narrow, f'golden mask as {values.dtype}, narrow={narrow}')
        raw, _ = _file_bytes(values, narrow)
        ratio = len(frag) / len(zlib.compress(raw, 1))
        print(f'golden mask as {values.dtype}, narrow={narrow}: {len(frag)} B, {ratio:.2f} x zlib level 1')
        assert ratio <= 2.0


def test_refused_calls_return_their_codes_and_launch_nothing():
    from fast_nnunet_amd import capi
    a = torch.arange(64, dtype=torch.uint8, device=DEV)
    cap = capi.deflate_bound(64)
    out = torch.full((cap + 16,), FILL, dtype=torch.uint8, device=DEV)
    host = np.zeros(256, np.uint8)

    def call(in_ptr=None, size=1, n=64, out_ptr=None, out_cap=cap):
        return capi.deflate_labels(a.data_ptr() if in_ptr is None else in_ptr, size, n, True,
                                   out.data_ptr() if out_ptr is None else out_ptr, out_cap)

    for match, kw, exc in (('NULL', dict(in_ptr=0), AssertionError), ('NULL', dict(out_ptr=0), AssertionError),
                           ('device', dict(in_ptr=host.ctypes.data - host.ctypes.data % 16 + 16), AssertionError),
                           ('device', dict(out_ptr=host.ctypes.data), AssertionError),
                           ('aligned', dict(in_ptr=a.data_ptr() + 8), AssertionError),
                           ('aligned', dict(in_ptr=a.data_ptr() + 2, size=2, n=16), AssertionError),
                           ('1 or 2', dict(size=0), AssertionError), ('1 or 2', dict(size=3), AssertionError),
                           ('1 or 2', dict(size=4, n=16), AssertionError), ('negative', dict(n=-1), AssertionError),
                           ('bound', dict(out_cap=cap - 1), AssertionError), ('bound', dict(out_cap=0), AssertionError),
                           ('too many', dict(n=2 ** 46), NotImplementedError),
                           ('too many', dict(n=2 ** 45, size=2), NotImplementedError)):
        with pytest.raises(exc, match=match):
            call(**kw)
        assert capi.op_last_kernels() == [], (kw, 'a refused call launches nothing')
    assert call(n=0) == (0, 1, 0) and capi.op_last_kernels() == [], 'no elements: nothing to do'
    assert capi.deflate_labels(a.data_ptr(), 2, 0, False, out.data_ptr(), 0) == (0, 2, 0)
    torch.cuda.synchronize()
    assert bool((out == FILL).all()) and bool((a == torch.arange(64, dtype=torch.uint8, device=DEV)).all())
    # 2^31 bytes are no limit of the interface: the refusal begins past 2^31 - 1 chunks
    assert capi.deflate_bound(2 ** 31 + 5) == (9 * (2 ** 31 + 5) + 7) // 8 + 6 * (2 ** 17 + 1)
    n_out, size, crc = call()
    assert size == 1 and deflate_ref.inflate(bytes(out[:n_out].cpu().numpy())) == bytes(range(64)) and crc == zlib.crc32(bytes(range(64)))


def test_every_kernel_is_launched():
    """Every instantiation csrc/deflate.hip holds, by the name ``fnn_op_last_kernels`` reports (``_deflate`` asserts the
    names of each call against the element sizes)."""
    from fast_nnunet_amd import capi
    seen = set()
    for values, narrow in ((np.arange(300, dtype=np.uint8), False), (np.arange(300, dtype=np.uint16), False),
                           (np.arange(300, dtype=np.uint16), True), (np.arange(200, dtype=np.uint16), True)):
        _check(values, narrow, f'{values.dtype}, narrow={narrow}')
        seen.update(capi.op_last_kernels())
    assert seen == {'deflate_max_kernel', 'deflate_scan_kernel', 'deflate_count_kernel<1,0>', 'deflate_emit_kernel<1,0>',
                    'deflate_count_kernel<2,0>', 'deflate_emit_kernel<2,0>', 'deflate_count_kernel<1,1>', 'deflate_emit_kernel<1,1>'}


# ---------------------------------------------------------------------------------------------------------------
# the reader-writers and the case pipeline
# ---------------------------------------------------------------------------------------------------------------
def _predictors(tmp, name):
    """The toy model folder of tests/test_gpu_predictor.py read by two predictors: the default and compress_on_device."""
    import json
    from fast_nnunet_amd import nnUNetPredictor
    folder, plans, dj, sd, spec = _toy_model_folder(tmp, PATCH, 3, plans_spacing=(3.0, 3.0, 3.0))
    if name is not None:
        (folder / 'dataset.json').write_text(json.dumps(dict(dj, overwrite_image_reader_writer=name)))
    made = []
    for flag in (False, True):
        p = nnUNetPredictor(tile_step_size=0.5, use_gaussian=True, use_mirroring=False, device=DEV, allow_tqdm=False,
                            patches_per_forward=4, compress_on_device=flag)
        p.initialize_from_trained_model_folder(str(folder), use_folds=(0,))
        made.append(p)
    return made


def _same_but_for_the_compressed_bytes(default_file, device_file):
    a, b = open(default_file, 'rb').read(), open(device_file, 'rb').read()
    assert gzip.decompress(a) == gzip.decompress(b), f'{device_file}: other header or voxels'
    assert a != b and a[:10] == b[:10], f'{device_file}: the device route was not taken'
    x, xi = nifti_ref.read(str(default_file))
    y, yi = nifti_ref.read(str(device_file))
    assert np.array_equal(x, y) and np.array_equal(xi['sform'], yi['sform'])
    return y


@pytest.mark.parametrize('name', (None, 'NibabelIOWithReorient'), ids=('NiftiIO', 'NibabelIOWithReorient'))
def test_pipeline_with_compress_on_device_writes_the_same_files(tmp_path, name):
    from fast_nnunet_amd.imageio import DeviceCompressedLabels, NiftiIO, NiftiReorientIO
    default, device = _predictors(tmp_path, name)
    assert type(device._reader_writer()) is (NiftiIO if name is None else NiftiReorientIO) and device.compress_on_device
    src = tmp_path / 'in'
    src.mkdir()
    perm, signs = TRANSPOSE_ORIENTATION
    n = 3
    for i in range(n):
        _oriented_file(str(src / f'c{i}_0000.nii.gz'), _small_ras(70 + i), 4, perm, signs)
    out = {k: tmp_path / k for k in ('default', 'threads', 'inline', 'sequential')}
    assert default.predict_from_files(str(src), str(out['default'])) == [None] * n
    assert device.predict_from_files(str(src), str(out['threads']), num_processes_preprocessing=2,
                                     num_processes_segmentation_export=2) == [None] * n
    assert device.predict_from_files(str(src), str(out['inline']), num_processes_preprocessing=0,
                                     num_processes_segmentation_export=0) == [None] * n
    assert device.predict_from_files_sequential(str(src), str(out['sequential'])) == [None] * n
    classes = set()
    for i in range(n):
        for k in ('threads', 'inline', 'sequential'):
            classes.update(np.unique(_same_but_for_the_compressed_bytes(out['default'] / f'c{i}.nii.gz', out[k] / f'c{i}.nii.gz')))
    assert len(classes) >= 2, 'label maps with more than background'
    for i in range(n):
        assert open(out['threads'] / f'c{i}.nii.gz', 'rb').read() == open(out['inline'] / f'c{i}.nii.gz', 'rb').read() \
            == open(out['sequential'] / f'c{i}.nii.gz', 'rb').read(), 'the same bytes whichever thread writes them'
    # predict_single_npy_array with an output file, probabilities next to it; returned arrays are untouched
    rw = device._reader_writer()
    img, props = rw.read_images([str(src / 'c0_0000.nii.gz')], on_device=False)
    assert device.predict_single_npy_array(img, props, output_file_truncated=str(tmp_path / 'single'),
                                           save_or_return_probabilities=True) is None
    assert default.predict_single_npy_array(img, props, output_file_truncated=str(tmp_path / 'single_default'),
                                            save_or_return_probabilities=True) is None
    _same_but_for_the_compressed_bytes(tmp_path / 'single_default.nii.gz', tmp_path / 'single.nii.gz')
    assert open(tmp_path / 'single.nii.gz', 'rb').read() == open(out['threads'] / 'c0.nii.gz', 'rb').read()
    assert np.array_equal(np.load(tmp_path / 'single.npz')['probabilities'], np.load(tmp_path / 'single_default.npz')['probabilities'])
    assert open(tmp_path / 'single.pkl', 'rb').read() == open(tmp_path / 'single_default.pkl', 'rb').read()
    seg = device.predict_single_npy_array(img, props)
    assert isinstance(seg, np.ndarray) and np.array_equal(seg, default.predict_single_npy_array(img, props))
    assert np.array_equal(device.predict_from_files([[str(src / 'c0_0000.nii.gz')]], None)[0], seg)
    # the reader-writer's own method: a device tensor in, the value write_seg takes out; a numpy array takes today's route
    labels = rw.compress_labels(torch.from_numpy(seg).to(DEV), props)
    assert isinstance(labels, DeviceCompressedLabels) and not labels.uint16 and labels.n_bytes == seg.size
    rw.write_seg(labels, str(tmp_path / 'own.nii.gz'), props)
    assert open(tmp_path / 'own.nii.gz', 'rb').read() == open(out['threads'] / 'c0.nii.gz', 'rb').read()
    rw.write_seg(seg, str(tmp_path / 'numpy.nii.gz'), props)
    assert open(tmp_path / 'numpy.nii.gz', 'rb').read() == open(out['default'] / 'c0.nii.gz', 'rb').read()
    wide = rw.compress_labels(torch.from_numpy(seg.astype(np.int16) * 200).to(DEV), props)         # maximum 400: a uint16 file
    rw.write_seg(wide, str(tmp_path / 'wide.nii.gz'), props)
    rw.write_seg(seg.astype(np.uint16) * 200, str(tmp_path / 'wide_numpy.nii.gz'), props)
    assert wide.uint16 and gzip.decompress(open(tmp_path / 'wide.nii.gz', 'rb').read()) == \
        gzip.decompress(open(tmp_path / 'wide_numpy.nii.gz', 'rb').read())
    assert not [t.name for t in threading.enumerate() if t.name.startswith('fnn-')], 'reader and writer threads have ended'
    left = [f for d, _, fs in os.walk(tmp_path) for f in fs if '.part' in f]
    assert not left, left
