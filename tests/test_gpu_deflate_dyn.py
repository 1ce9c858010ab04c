"""The device deflate encoder with per-chunk dynamic Huffman tables on a real MI355X: ``fnn_deflate_labels_dyn`` against
zlib's inflate, ``zlib.crc32`` and the Python model of its rule (tests/deflate_dyn_ref.py) byte for byte, and the case
pipeline with ``compress_on_device='dynamic'`` against the default and the fixed-code routes.

Kernels launched here (csrc/deflate_dyn.hip): deflate_dyn_count_kernel / deflate_dyn_emit_kernel <1,0> (uint8), <2,0>
(uint16) and <1,1> (a two-byte map written as uint8), with deflate.hip's deflate_max_kernel and deflate_scan_kernel -
``test_every_kernel_is_launched`` reads their names from ``fnn_op_last_kernels``.  Contents, lengths and canaries are those
of tests/test_gpu_deflate.py: lengths around the segment (256 bytes, one lane) and the chunk (16 KiB, one wave), the largest
40 chunks + 123 elements; ``out`` starts at an odd address between canaries.  The length limit of 15 is reached by the
Fibonacci chunk and the limit of 7 of the header's code by ``deep_header_chunk`` (tests/test_deflate_dyn_cpu.py and
tests/test_deflate_dyn_host_cpu.py say why), the fixed-code choice by the tiny chunk.
"""
import gzip
import os
import threading
import zlib

import numpy as np
import pytest
import torch

import deflate_dyn_ref as dyn
import deflate_ref
import nifti_ref
from test_gpu_deflate import BACK, C, CONTENTS, DEV, FILL, FRONT, LENGTHS, MASK, _file_bytes
from test_gpu_predictor import _toy_model_folder
from test_gpu_reorient import PATCH, TRANSPOSE_ORIENTATION, _oriented_file, _small_ras

pytestmark = pytest.mark.gpu


def _deflate(values, narrow, aligned_out=False):
    """-> (fragment bytes, bytes per element in the file, crc, dynamic chunks) of one call, with every check that needs the
    device buffer."""
    from fast_nnunet_amd import capi
    size = values.dtype.itemsize
    src = torch.from_numpy(values.view(np.uint8).copy()).to(DEV) if values.size else torch.zeros(16, dtype=torch.uint8, device=DEV)
    assert src.data_ptr() % 16 == 0
    cap = capi.deflate_bound(values.size * size)
    front = 64 if aligned_out else FRONT
    buf = torch.full((front + cap + BACK,), FILL, dtype=torch.uint8, device=DEV)
    n_out, file_size, crc, dynamic_chunks = capi.deflate_labels_dyn(src.data_ptr(), size, values.size, narrow, buf.data_ptr() + front, cap,
                                                                    torch.cuda.current_stream(DEV).cuda_stream)
    want = [f'deflate_dyn_count_kernel<{file_size},{int(file_size != size)}>', 'deflate_scan_kernel',
            f'deflate_dyn_emit_kernel<{file_size},{int(file_size != size)}>'] if values.size else []
    assert capi.op_last_kernels() == (['deflate_max_kernel'] if narrow and size == 2 and values.size else []) + want
    host = buf.cpu().numpy()
    assert 0 <= n_out <= cap, f'{n_out} bytes, the bound is {cap}'
    assert np.all(host[:front] == FILL) and np.all(host[front + n_out:] == FILL), 'wrote outside out[0, out_bytes)'
    assert np.array_equal(src.cpu().numpy()[:values.size * size], values.view(np.uint8)), 'the input is left alone'
    return host[front:front + n_out].tobytes(), file_size, crc, dynamic_chunks


def _check(values, narrow, where, **kw):
    frag, file_size, crc, dynamic_chunks = _deflate(values, narrow, **kw)
    raw, want_size = _file_bytes(values, narrow)
    assert file_size == want_size, where
    d = zlib.decompressobj(-15)
    plain = d.decompress(frag + b'\x03\x00') + d.flush()
    assert d.eof and d.unused_data == b'' and plain == raw, f'{where}: inflate does not return the input'
    assert crc == zlib.crc32(raw), where
    want, want_dynamic = dyn.fragment(raw, file_size)
    if frag != want:
        i = next((k for k in range(min(len(frag), len(want))) if frag[k] != want[k]), min(len(frag), len(want)))
        raise AssertionError(f'{where}: {len(frag)} bytes, the model gives {len(want)}; first difference at byte {i}')
    assert dynamic_chunks == want_dynamic, where
    return frag, dynamic_chunks


@pytest.mark.parametrize('kind', list(CONTENTS))
def test_fragment_inflates_to_the_input_and_equals_the_model(kind):
    rng = np.random.default_rng(sorted(CONTENTS).index(kind))
    for n in LENGTHS:
        if kind == 'uint16_stays_with_255' and n < 2:
            continue
        values, narrow = CONTENTS[kind](rng, n)
        assert values.size == n
        first, _ = _check(values, narrow, f'{kind}, {n} elements')
        if n in (3, C + 1, LENGTHS[-1]):
            again = _deflate(values, narrow)[0]
            assert again == first, f'{kind}, {n} elements: two runs differ'
            aligned = _deflate(values, narrow, aligned_out=True)[0]
            assert aligned == first, f'{kind}, {n} elements: the bytes depend on where out lies'


def test_the_limits_and_the_choice():
    """The Fibonacci chunk (a tree 19 deep, cut at 15), the chunk whose header code is cut at 7 bits, the tiny chunk that
    takes the fixed code - alone and as neighbours in one map (padded to whole chunks with a label map's runs)."""
    fib, deep, tiny = (np.frombuffer(b, np.uint8) for b in (dyn.fibonacci_chunk(), dyn.deep_header_chunk(), dyn.TINY_CHUNK))
    assert max(dyn.tables(dyn.chunk_symbols(fib.tobytes(), 1))[0]) == 15
    assert max(dyn.code_lengths(dyn.header_code_frequencies(deep.tobytes(), 1), 15)) > 7
    assert _check(fib, False, 'the Fibonacci chunk')[1] == 1
    assert _check(deep, False, 'the chunk with a deep header code')[1] == 1
    frag, dynamic_chunks = _check(tiny, False, 'the tiny chunk')
    assert dynamic_chunks == 0 and frag == deflate_ref.fragment(tiny.tobytes(), 1)

    def whole(a):
        return np.concatenate([a, np.repeat(np.arange(40, dtype=np.uint8) % 4, 500)[:C - a.size]])
    assert _check(np.concatenate([whole(fib), whole(deep), tiny]), False, 'the three as neighbours')[1] == 2


def test_golden_mask_and_the_size_condition(golden_dir):
    """At most 1.0 x zlib level 1, what the host writer makes by default."""
    voxels = np.frombuffer(gzip.decompress(open(os.path.join(golden_dir, MASK), 'rb').read())[352:], np.uint8)
    for values, narrow in ((voxels, False), (voxels.astype(np.uint16), False)):
        frag, dynamic_chunks = _check(values, narrow, f'golden mask as {values.dtype}')
        raw, _ = _file_bytes(values, narrow)
        ratio = len(frag) / len(zlib.compress(raw, 1))
        print(f'golden mask as {values.dtype}: {len(frag)} B in {dynamic_chunks} dynamic chunks, {ratio:.2f} x zlib level 1')
        assert ratio <= 1.0


def test_refused_calls_return_their_codes_and_launch_nothing():
    from fast_nnunet_amd import capi
    a = torch.arange(64, dtype=torch.uint8, device=DEV)
    cap = capi.deflate_bound(64)
    out = torch.full((cap + 16,), FILL, dtype=torch.uint8, device=DEV)
    host = np.zeros(256, np.uint8)

    def call(in_ptr=None, size=1, n=64, out_ptr=None, out_cap=cap):
        return capi.deflate_labels_dyn(a.data_ptr() if in_ptr is None else in_ptr, size, n, True,
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
    assert call(n=0) == (0, 1, 0, 0) and capi.op_last_kernels() == [], 'no elements: nothing to do'
    assert capi.deflate_labels_dyn(a.data_ptr(), 2, 0, False, out.data_ptr(), 0) == (0, 2, 0, 0)
    torch.cuda.synchronize()
    assert bool((out == FILL).all()) and bool((a == torch.arange(64, dtype=torch.uint8, device=DEV)).all())
    n_out, size, crc, dynamic_chunks = call()
    assert size == 1 and deflate_ref.inflate(bytes(out[:n_out].cpu().numpy())) == bytes(range(64)) and crc == zlib.crc32(bytes(range(64)))
    assert dynamic_chunks == 0, '64 distinct bytes: a table header costs more than it saves'
    # dynamic_chunks may be NULL
    import ctypes as ct
    lib = capi.load_library()
    n_b, elem_b, crc_b = ct.c_int64(-1), ct.c_int(0), ct.c_uint32(0)
    assert lib.fnn_deflate_labels_dyn(a.data_ptr(), 1, 64, 1, out.data_ptr(), cap, ct.byref(n_b), ct.byref(elem_b), ct.byref(crc_b), None, None) == 0
    assert (n_b.value, elem_b.value, crc_b.value) == (n_out, 1, crc)


def test_every_kernel_is_launched():
    """Every instantiation csrc/deflate_dyn.hip holds, by the name ``fnn_op_last_kernels`` reports (``_deflate`` asserts the
    names of each call against the element sizes); 20 000 elements of a few labels: both chunks take their own tables."""
    from fast_nnunet_amd import capi
    seen = set()
    base = np.arange(20000) // 70 % 6
    for values, narrow in ((base.astype(np.uint8), False), ((base * 300).astype(np.uint16), False),
                           ((base * 300).astype(np.uint16), True), (base.astype(np.uint16), True)):
        assert _check(values, narrow, f'{values.dtype}, narrow={narrow}')[1] == -(-values.size * (2 if values.max() > 255 else 1) // C)
        seen.update(capi.op_last_kernels())
    assert seen == {'deflate_max_kernel', 'deflate_scan_kernel', 'deflate_dyn_count_kernel<1,0>', 'deflate_dyn_emit_kernel<1,0>',
                    'deflate_dyn_count_kernel<2,0>', 'deflate_dyn_emit_kernel<2,0>', 'deflate_dyn_count_kernel<1,1>', 'deflate_dyn_emit_kernel<1,1>'}


# ---------------------------------------------------------------------------------------------------------------
# the reader-writers and the case pipeline
# ---------------------------------------------------------------------------------------------------------------
def _predictors(tmp):
    """The toy model folder of tests/test_gpu_predictor.py read by three predictors: the default, the fixed code, dynamic."""
    from fast_nnunet_amd import nnUNetPredictor
    folder, plans, dj, sd, spec = _toy_model_folder(tmp, PATCH, 3, plans_spacing=(3.0, 3.0, 3.0))
    made = []
    for flag in (False, True, 'dynamic'):
        p = nnUNetPredictor(tile_step_size=0.5, use_gaussian=True, use_mirroring=False, device=DEV, allow_tqdm=False,
                            patches_per_forward=4, compress_on_device=flag)
        assert p.compress_on_device is flag or p.compress_on_device == flag == 'dynamic'
        p.initialize_from_trained_model_folder(str(folder), use_folds=(0,))
        made.append(p)
    return made, plans, dj


def test_pipeline_with_dynamic_tables_writes_the_same_voxels_in_smaller_files(tmp_path):
    from fast_nnunet_amd import postprocessing as pp
    from fast_nnunet_amd.ensembling import nnUNetEnsemblePredictor
    from fast_nnunet_amd.jhu import JHUPredictor
    from fast_nnunet_amd.imageio import DeviceCompressedLabels, NiftiIO, chunked_layout, read_header
    (default, fixed, dynamic), plans, dj = _predictors(tmp_path)
    src = tmp_path / 'in'
    src.mkdir()
    perm, signs = TRANSPOSE_ORIENTATION
    n = 2
    for i in range(n):
        _oriented_file(str(src / f'c{i}_0000.nii.gz'), _small_ras(70 + i), 4, perm, signs)
    out = {k: tmp_path / k for k in ('default', 'fixed', 'threads', 'inline', 'sequential')}
    assert default.predict_from_files(str(src), str(out['default'])) == [None] * n
    assert fixed.predict_from_files(str(src), str(out['fixed'])) == [None] * n
    assert dynamic.predict_from_files(str(src), str(out['threads']), num_processes_preprocessing=2,
                                      num_processes_segmentation_export=2) == [None] * n
    assert dynamic.predict_from_files(str(src), str(out['inline']), num_processes_preprocessing=0,
                                      num_processes_segmentation_export=0) == [None] * n
    assert dynamic.predict_from_files_sequential(str(src), str(out['sequential'])) == [None] * n
    for i in range(n):
        files = {k: open(out[k] / f'c{i}.nii.gz', 'rb').read() for k in out}
        assert gzip.decompress(files['threads']) == gzip.decompress(files['default']), 'the same header and voxels'
        assert files['threads'][:10] == files['default'][:10] and files['threads'] != files['fixed']
        assert len(files['threads']) <= len(files['fixed']), 'no longer than the fixed code\'s file'
        assert files['threads'] == files['inline'] == files['sequential'], 'the same bytes whichever thread writes them'
        x, xi = nifti_ref.read(str(out['default'] / f'c{i}.nii.gz'))
        y, yi = nifti_ref.read(str(out['threads'] / f'c{i}.nii.gz'))
        assert np.array_equal(x, y) and np.array_equal(xi['sform'], yi['sform'])
    # reading back: the file is still laid out in chunks, the device decoder refuses its dynamic blocks, zlib reads it
    name = str(out['threads'] / 'c0.nii.gz')
    assert chunked_layout(open(name, 'rb').read(), read_header(name)) is not None
    reader = NiftiIO(DEV, inflate_on_device=True)
    got, _ = reader.read_label_map(name)
    plain, _ = NiftiIO(DEV).read_label_map(name)
    assert torch.equal(got, plain) and reader.inflate_stats == {'device': 0, 'host': 0, 'fallback': 1}
    seg, _ = reader.read_seg(name)                               # (read_seg decodes images: it never takes the device inflate)
    assert np.array_equal(seg.cpu().numpy()[0].astype(np.uint8), plain.cpu().numpy())
    assert reader.inflate_stats == {'device': 0, 'host': 0, 'fallback': 1}, 'read_seg leaves the counts alone'
    # the reader-writer's own method
    rw = dynamic._reader_writer()
    labels = rw.compress_labels(plain, NiftiIO(DEV).read_label_map(name)[1], tables='dynamic')
    again = rw.compress_labels(plain, NiftiIO(DEV).read_label_map(name)[1], 'fixed')
    assert isinstance(labels, DeviceCompressedLabels) and labels.n_bytes == again.n_bytes == plain.numel()
    with pytest.raises(ValueError, match='tables'):
        rw.compress_labels(plain, {}, tables='best')
    # the switch: anything but False, True and 'dynamic' is refused at construction; the mask encoder has no dynamic tables
    from fast_nnunet_amd import nnUNetPredictor
    for bad in ('fixed', 'Dynamic', 2, None, 1.5):
        with pytest.raises(ValueError, match='compress_on_device'):
            nnUNetPredictor(device=DEV, allow_tqdm=False, compress_on_device=bad)
        with pytest.raises(ValueError, match='compress_on_device'):
            nnUNetEnsemblePredictor([default], compress_on_device=bad)
        with pytest.raises(ValueError, match='compress_on_device'):
            pp.apply_postprocessing_to_folder(str(out['threads']), str(tmp_path / 'never'), [], [], compress_on_device=bad)
        with pytest.raises(ValueError, match='compress_on_device'):
            pp.load_postprocess_save(name, str(tmp_path / 'never.nii.gz'), NiftiIO(DEV), [], [], compress_on_device=bad)
    assert not os.path.exists(tmp_path / 'never') and not os.path.exists(tmp_path / 'never.nii.gz')
    with pytest.raises(NotImplementedError, match='mask encoder'):
        JHUPredictor(device=DEV, allow_tqdm=False, compress_on_device='dynamic')
    assert JHUPredictor(device=DEV, allow_tqdm=False, compress_on_device=True).compress_on_device is True
    # the ensemble and the folder command take the value
    def smaller_and_the_same(dyn_file, fixed_file):
        a, b = open(dyn_file, 'rb').read(), open(fixed_file, 'rb').read()
        assert gzip.decompress(a) == gzip.decompress(b) and a != b and len(a) <= len(b), dyn_file

    for flag in (True, 'dynamic'):
        ens = nnUNetEnsemblePredictor([default], compress_on_device=flag)
        assert ens.compress_on_device == flag
        assert ens.predict_from_files(str(src), str(tmp_path / f'ens_{flag}')) == [None] * n
        pp.apply_postprocessing_to_folder(str(out['default']), str(tmp_path / f'pp_{flag}'), [], [], plans, dj, compress_on_device=flag)
        pp.load_postprocess_save(str(out['default'] / 'c1.nii.gz'), str(tmp_path / f'one_{flag}.nii.gz'), NiftiIO(DEV), [], [],
                                 compress_on_device=flag)
    for i in range(n):
        smaller_and_the_same(tmp_path / 'ens_dynamic' / f'c{i}.nii.gz', tmp_path / 'ens_True' / f'c{i}.nii.gz')
        smaller_and_the_same(tmp_path / 'pp_dynamic' / f'c{i}.nii.gz', tmp_path / 'pp_True' / f'c{i}.nii.gz')
        assert gzip.decompress(open(tmp_path / 'pp_dynamic' / f'c{i}.nii.gz', 'rb').read()) == gzip.decompress(open(out['default'] / f'c{i}.nii.gz', 'rb').read())
    smaller_and_the_same(tmp_path / 'one_dynamic.nii.gz', tmp_path / 'one_True.nii.gz')
    assert not [t.name for t in threading.enumerate() if t.name.startswith('fnn-')], 'reader and writer threads have ended'
    left = [f for d, _, fs in os.walk(tmp_path) for f in fs if '.part' in f]
    assert not left, left
