"""Reorientation on a real MI355X: ``fnn_reorient`` against numpy's flip and transpose bit for bit, ``NiftiReorientIO`` on the
device against its numpy route, and the case pipeline with ``overwrite_image_reader_writer: 'NibabelIOWithReorient'``.

Kernels launched here (csrc/reorient.hip): reorient_rows_kernel<1>, <2>, <4> (``src_axis[2] == 2``) and
reorient_transpose_kernel<1>, <2>, <4> (every other ``src_axis``) - all 48 ``(src_axis, flip)`` pairs per element size, on
shapes around the transposed path's tile edge T = 64, with both buffers one element past an aligned base between canaries.
"""
import gzip
import itertools
import os
import pickle
import shutil
import threading

import numpy as np
import pytest
import torch

import nifti_ref
import orient_ref
from test_gpu_predictor import _toy_model_folder

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda', 0)
CT = 'example_ct_sm.nii.gz'
T = 64                                                            # RO_TILE of csrc/reorient.hip
SHAPES = [(1, 1, 1), (3, 5, 7), (2, T + 5, 2 * T + 3), (T + 5, 2 * T + 3, 2), (2 * T + 3, 2, T + 5), (1, 4 * T + 1, 1)]
PAIRS = [(p, f) for p in itertools.permutations(range(3)) for f in itertools.product((0, 1), repeat=3)]
CANARY = 16                                                       # elements in front of and behind each array
DTYPE_OF = {1: np.uint8, 2: np.uint16, 4: np.uint32}


def _numpy_reorient(a, src_axis, flip):
    """out[i] = a[j], j[src_axis[d]] = shape[src_axis[d]] - 1 - i[d] where flip[d], else i[d]."""
    t = a.transpose(src_axis)
    axes = tuple(d for d in range(3) if flip[d])
    return np.ascontiguousarray(np.flip(t, axes) if axes else t)


def test_numpy_reorient_is_the_issues_formula():
    a = np.arange(2 * 3 * 4).reshape(2, 3, 4)
    for src, flip in PAIRS:
        out = _numpy_reorient(a, src, flip)
        assert out.shape == tuple(a.shape[s] for s in src)
        for i in np.ndindex(*out.shape):
            j = [0, 0, 0]
            for d in range(3):
                j[src[d]] = a.shape[src[d]] - 1 - i[d] if flip[d] else i[d]
            assert out[i] == a[tuple(j)]


# ---------------------------------------------------------------------------------------------------------------
# fnn_reorient
# ---------------------------------------------------------------------------------------------------------------
def _placed(values, dt, fill):
    """`values` (flat) on the device one element past a 16-byte aligned base, CANARY elements of `fill` on each side;
    -> (the whole buffer, the byte offset of the first value)."""
    n = values.size
    host = np.full(n + 2 * CANARY + 1, fill, dtype=dt)
    host[CANARY + 1:CANARY + 1 + n] = values
    buf = torch.from_numpy(host.view(np.uint8).copy()).to(DEV)
    assert buf.data_ptr() % 16 == 0
    return buf, (CANARY + 1) * np.dtype(dt).itemsize


@pytest.mark.parametrize('size', (1, 2, 4), ids=['reorient<1>', 'reorient<2>', 'reorient<4>'])
def test_reorient_matches_numpy_bit_for_bit(size):
    from fast_nnunet_amd import capi
    dt = np.dtype(DTYPE_OF[size])
    info = np.iinfo(dt)
    fill_in, fill_out = dt.type(info.max - 2), dt.type(info.max - 5)
    stream = torch.cuda.current_stream(DEV).cuda_stream
    rng = np.random.default_rng(size)
    done = {'rows': 0, 'transpose': 0}
    for shape in SHAPES:
        n = int(np.prod(shape))
        a = rng.integers(0, int(info.max) + 1, shape, dtype=np.uint64).astype(dt)
        src_buf, src_off = _placed(a.reshape(-1), dt, fill_in)
        launched = []
        for src, flip in PAIRS:
            dst_buf, dst_off = _placed(np.full(n, fill_out, dtype=dt), dt, fill_out)
            capi.reorient(src_buf.data_ptr() + src_off, size, shape, src, flip, dst_buf.data_ptr() + dst_off, stream)
            launched.append((src, flip, dst_buf))
        host_src = src_buf.cpu().numpy().view(dt)
        assert np.array_equal(host_src[CANARY + 1:CANARY + 1 + n], a.reshape(-1)) and np.all(host_src[:CANARY + 1] == fill_in) \
            and np.all(host_src[CANARY + 1 + n:] == fill_in), 'the input is left alone'
        for src, flip, dst_buf in launched:
            got = dst_buf.cpu().numpy().view(dt)
            want = _numpy_reorient(a, src, flip).reshape(-1)
            where = f'elem_bytes={size} shape={shape} src_axis={src} flip={flip}'
            assert np.all(got[:CANARY + 1] == fill_out) and np.all(got[CANARY + 1 + n:] == fill_out), f'{where}: wrote outside out'
            diff = got[CANARY + 1:CANARY + 1 + n] != want
            if diff.any():
                i = int(np.flatnonzero(diff)[0])
                raise AssertionError(f'{where}: element {i} is {got[CANARY + 1 + i]}, numpy gives {want[i]}; '
                                     f'{int(diff.sum())} of {n} differ')
            done['rows' if src[2] == 2 else 'transpose'] += 1
    assert done == {'rows': 16 * len(SHAPES), 'transpose': 32 * len(SHAPES)}
    print(f'reorient_rows_kernel<{size}>: {done["rows"]} launches, reorient_transpose_kernel<{size}>: {done["transpose"]} '
          f'launches bit-identical to numpy')


def test_reorient_with_aligned_buffers_and_rows_longer_than_a_chunk():
    """The 16-byte loads and stores of the rows path (aligned rows), and its funnel-shifted ones (rows of 1- and 2-byte
    elements that start off a dword), with rows long enough to hold whole chunks."""
    from fast_nnunet_amd import capi
    for size, shape in ((1, (3, 4, 64)), (2, (3, 4, 32)), (4, (3, 4, 16)), (1, (2, 3, 71)), (2, (2, 3, 37)), (4, (2, 3, 19))):
        dt = np.dtype(DTYPE_OF[size])
        a = np.random.default_rng(7).integers(0, int(np.iinfo(dt).max) + 1, shape, dtype=np.uint64).astype(dt)
        src_t = torch.from_numpy(a.view(np.uint8).copy()).to(DEV)
        for src, flip in PAIRS:
            out = torch.zeros(a.size * size, dtype=torch.uint8, device=DEV)
            capi.reorient(src_t.data_ptr(), size, shape, src, flip, out.data_ptr())
            got = out.cpu().numpy().view(dt)
            assert np.array_equal(got, _numpy_reorient(a, src, flip).reshape(-1)), (size, shape, src, flip)


def test_reorient_refuses_what_it_cannot_serve():
    from fast_nnunet_amd import capi
    a = torch.arange(64, dtype=torch.uint8, device=DEV)
    out = torch.full((64,), 7, dtype=torch.uint8, device=DEV)
    ok = dict(elem_bytes=1, shape_in=(2, 3, 4), src_axis=(2, 0, 1), flip=(1, 0, 1))

    def call(in_ptr=None, out_ptr=None, **kw):
        k = dict(ok, **kw)
        capi.reorient(a.data_ptr() if in_ptr is None else in_ptr, k['elem_bytes'], k['shape_in'], k['src_axis'], k['flip'],
                      out.data_ptr() if out_ptr is None else out_ptr)

    with pytest.raises(AssertionError, match='NULL'):
        call(in_ptr=0)
    with pytest.raises(AssertionError, match='NULL'):
        call(out_ptr=0)
    host = np.zeros(64, np.uint8)
    with pytest.raises(AssertionError, match='device'):
        call(in_ptr=host.ctypes.data)
    with pytest.raises(AssertionError, match='device'):
        call(out_ptr=host.ctypes.data)
    for size in (0, 3, 8, -1):
        with pytest.raises(NotImplementedError, match='1, 2 or 4'):
            call(elem_bytes=size)
    for src in ((0, 0, 1), (0, 1, 3), (-1, 1, 2), (2, 2, 2)):
        with pytest.raises(AssertionError, match='permutation'):
            call(src_axis=src)
    with pytest.raises(AssertionError, match='extent'):
        call(shape_in=(2, -3, 4))
    with pytest.raises(AssertionError, match='aligned'):
        call(elem_bytes=2, in_ptr=a.data_ptr() + 1)
    with pytest.raises(AssertionError, match='overlap'):
        call(out_ptr=a.data_ptr() + 23)
    with pytest.raises(AssertionError, match='overlap'):
        call(in_ptr=a.data_ptr() + 8, out_ptr=a.data_ptr())
    with pytest.raises(NotImplementedError, match='too many'):
        call(shape_in=(2 ** 40, 2 ** 30, 4), out_ptr=out.data_ptr())
    with pytest.raises(NotImplementedError, match='too many'):                # the transposed path's tiles: more blocks than a launch has
        call(shape_in=(2 ** 31, 2 ** 10, 1), src_axis=(2, 1, 0), in_ptr=a.data_ptr(), out_ptr=a.data_ptr() + 2 ** 42)
    call(shape_in=(2, 0, 4))                                                     # no elements: nothing to do
    call(in_ptr=a.data_ptr(), out_ptr=a.data_ptr() + 24)                         # adjacent ranges do not overlap
    torch.cuda.synchronize()
    assert bool((out == 7).all()) and bool((a[:24] == torch.arange(24, dtype=torch.uint8, device=DEV)).all()), \
        'a refused or empty call writes nothing'
    assert bool((a[24:48].cpu() == torch.from_numpy(_numpy_reorient(np.arange(24, dtype=np.uint8).reshape(2, 3, 4),
                                                                      (2, 0, 1), (1, 0, 1)).reshape(-1))).all())


# ---------------------------------------------------------------------------------------------------------------
# NiftiReorientIO on the device against its numpy route
# ---------------------------------------------------------------------------------------------------------------
ROWS_ORIENTATION = ((0, 2, 1), (-1, 1, 1))                        # x stays the fastest axis: the row path, rows reversed
TRANSPOSE_ORIENTATION = ((2, 0, 1), (1, -1, 1))                   # the fastest axis moves: the tiled transpose
RAS_AFFINE = np.array([[3.0, 0, 0, -10.0], [0, 3.0, 0, 20.5], [0, 0, 3.0, 3.0], [0, 0, 0, 1.0]])


def _oriented_file(fname, ras_values, datatype, perm, signs, ras_affine=RAS_AFFINE, **kw):
    """`ras_values` (z, y, x) stored the way a scanner with orientation (perm, signs) would have: the voxels moved by
    orient_ref's inverse, the affine that places every voxel where `ras_affine` places it in the RAS array."""
    inv = orient_ref.invert(orient_ref.ornt_of(perm, signs))
    stored = orient_ref.apply_zyx(ras_values, inv)
    affine = ras_affine @ orient_ref.index_map(inv, ras_values.shape[::-1])
    zooms = np.sqrt((affine[:3, :3] ** 2).sum(0))
    nifti_ref.write(fname, stored, datatype, sform=affine, sform_code=2, pixdim=(1, *zooms), **kw)
    return affine


def _bits32(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize('perm, signs', (ROWS_ORIENTATION, TRANSPOSE_ORIENTATION, ((0, 1, 2), (1, 1, 1))),
                         ids=('rows', 'transpose', 'identity'))
def test_device_route_equals_numpy_route(tmp_path, perm, signs):
    from fast_nnunet_amd.imageio import NiftiReorientIO
    rng = np.random.default_rng(11)
    shape = (9, 11, 13)                                           # odd voxel count: the second channel starts off a 16-byte boundary
    a = (rng.standard_normal(shape) * 300).astype(np.int16)
    b = rng.integers(0, 256, shape).astype(np.uint8)
    files = [str(tmp_path / 'p_0000.nii.gz'), str(tmp_path / 'p_0001.nii.gz')]
    _oriented_file(files[0], a, 4, perm, signs)
    _oriented_file(files[1], b, 2, perm, signs, order='>', slope=0.5, inter=-3.0)
    rw = NiftiReorientIO(DEV)
    got, props = rw.read_images(files)
    want, want_props = rw.read_images(files, on_device=False)
    assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == (2, *shape) and (9 * 11 * 13) % 4 == 3
    assert np.array_equal(_bits32(got.cpu().numpy()), _bits32(want))
    assert np.array_equal(want[0], a.astype(np.float32)) and np.array_equal(want[1], np.float32(b * 0.5 - 3.0))
    assert props['spacing'] == want_props['spacing'] == [3.0, 3.0, 3.0] and sorted(props) == ['nibabel_stuff', 'spacing']
    for k in ('original_affine', 'reoriented_affine'):
        assert np.array_equal(props['nibabel_stuff'][k], want_props['nibabel_stuff'][k])
    assert np.allclose(props['nibabel_stuff']['reoriented_affine'], RAS_AFFINE)
    # labels: the device route of write_seg and read_seg against the numpy ones
    seg = rng.integers(0, 5, shape).astype(np.uint8)
    for name, labels in (('dev', torch.from_numpy(seg).to(DEV)), ('host', seg), ('dev16', torch.from_numpy(seg.astype(np.int16) * 100).to(DEV))):
        rw.write_seg(labels, str(tmp_path / f'{name}.nii.gz'), props)
    assert open(tmp_path / 'dev.nii.gz', 'rb').read() == open(tmp_path / 'host.nii.gz', 'rb').read()
    stored, info = nifti_ref.read(str(tmp_path / 'dev.nii.gz'))
    assert np.array_equal(stored, orient_ref.apply_zyx(seg, orient_ref.invert(orient_ref.ornt_of(perm, signs))))
    assert np.array_equal(info['sform'].astype(np.float32), props['nibabel_stuff']['original_affine'].astype(np.float32))
    stored16, info16 = nifti_ref.read(str(tmp_path / 'dev16.nii.gz'))
    assert int(info16['header']['datatype']) == 512 and np.array_equal(stored16, stored.astype(np.float32) * 100)
    back, _ = rw.read_seg(str(tmp_path / 'dev.nii.gz'))
    assert np.array_equal(back.cpu().numpy()[0], seg)


# ---------------------------------------------------------------------------------------------------------------
# the case pipeline
# ---------------------------------------------------------------------------------------------------------------
PATCH = (16, 16, 32)
SIX = [((0, 1, 2), (1, 1, 1)), ((0, 2, 1), (-1, 1, 1)), ((1, 0, 2), (1, -1, 1)), ((1, 2, 0), (1, 1, -1)), ((2, 0, 1), (-1, -1, 1)),
       ((2, 1, 0), (-1, -1, -1))]                                  # one per axis permutation, different flips


def _toy(tmp, name=None):
    """The toy model folder of tests/test_gpu_imageio.py; with `name` the dataset names its reader-writer."""
    import json
    from fast_nnunet_amd import nnUNetPredictor
    folder, plans, dj, sd, spec = _toy_model_folder(tmp, PATCH, 3, plans_spacing=(3.0, 3.0, 3.0))
    if name is not None:
        (folder / 'dataset.json').write_text(json.dumps(dict(dj, overwrite_image_reader_writer=name)))
    p = nnUNetPredictor(tile_step_size=0.5, use_gaussian=True, use_mirroring=False, device=DEV, allow_tqdm=False,
                        patches_per_forward=4)
    p.initialize_from_trained_model_folder(str(folder), use_folds=(0,))
    return p


@pytest.fixture(scope='module')
def toy(tmp_path_factory):
    return _toy(tmp_path_factory.mktemp('toy_reorient'), 'NibabelIOWithReorient')


@pytest.fixture(scope='module')
def toy_plain(tmp_path_factory):
    return _toy(tmp_path_factory.mktemp('toy_plain'))


def test_ct_fixture_in_six_orientations_end_to_end(toy, toy_plain, tmp_path, golden_dir):
    from fast_nnunet_amd.imageio import NiftiReorientIO, NiftiIO
    assert isinstance(toy._reader_writer(), NiftiReorientIO) and type(toy_plain._reader_writer()) is NiftiIO
    values, info = nifti_ref.read(os.path.join(golden_dir, CT))
    assert np.array_equal(values, values.astype(np.int16)), 'the fixture holds whole numbers: stored as int16 below'
    src, out = tmp_path / 'in', tmp_path / 'out'
    src.mkdir()
    affines = {}
    for k, (perm, signs) in enumerate(SIX):
        affines[k] = _oriented_file(str(src / f'o{k}_0000.nii.gz'), values.astype(np.int16), 4, perm, signs, ras_affine=info['affine'])
    assert toy.predict_from_files(str(src), str(out), num_processes_preprocessing=2, num_processes_segmentation_export=2) == [None] * 6
    ras_labels, ras_info = nifti_ref.read(str(out / 'o0.nii.gz'))
    assert len(np.unique(ras_labels)) >= 2 and ras_labels.shape == values.shape
    for k, (perm, signs) in enumerate(SIX):
        labels, linfo = nifti_ref.read(str(out / f'o{k}.nii.gz'))
        stored, sinfo = nifti_ref.read(str(src / f'o{k}_0000.nii.gz'))
        assert tuple(linfo['header']['dim'][1:4]) == tuple(sinfo['header']['dim'][1:4]), (k, 'the input file\'s dims')
        assert np.array_equal(linfo['sform'].astype(np.float32), sinfo['sform'].astype(np.float32)), (k, 'the input file\'s sform')
        assert np.array_equal(orient_ref.apply_zyx(labels, orient_ref.ornt_of(perm, signs)), ras_labels), \
            f'orientation {perm} {signs}: labels differ from the RAS run'
    # the identity case is byte for byte what NiftiIO writes
    plain_src, plain_out = tmp_path / 'plain_in', tmp_path / 'plain_out'
    plain_src.mkdir()
    shutil.copy(src / 'o0_0000.nii.gz', plain_src / 'o0_0000.nii.gz')
    assert toy_plain.predict_from_files(str(plain_src), str(plain_out)) == [None]
    assert open(plain_out / 'o0.nii.gz', 'rb').read() == open(out / 'o0.nii.gz', 'rb').read()
    assert not [t.name for t in threading.enumerate() if t.name.startswith('fnn-')]


def _small_ras(seed, shape=(18, 20, 36)):
    rng = np.random.default_rng(seed)
    v = (rng.standard_normal(shape) * 300 + 100).astype(np.int16)
    v[:2] = 0
    v[:, :, -3:] = 0
    return v


def test_returned_results_probabilities_and_single_array_export_stay_in_the_ras_frame(toy, tmp_path):
    from fast_nnunet_amd.imageio import NiftiReorientIO
    src, out = tmp_path / 'in', tmp_path / 'out'
    src.mkdir()
    perm, signs = TRANSPOSE_ORIENTATION
    f = str(src / 's_0000.nii.gz')
    _oriented_file(f, _small_ras(4), 4, perm, signs)
    img, props = NiftiReorientIO().read_images([f], on_device=False)
    assert np.array_equal(img[0], _small_ras(4).astype(np.float32))
    want_seg, want_probs = toy.predict_single_npy_array(img, props, save_or_return_probabilities=True)
    assert want_seg.shape == (18, 20, 36) and len(np.unique(want_seg)) >= 2
    # no output target: RAS-frame arrays come back
    ret = toy.predict_from_files([[f]], None, save_probabilities=True)
    assert np.array_equal(ret[0][0], want_seg) and np.array_equal(_bits32(ret[0][1]), _bits32(want_probs))
    assert np.array_equal(toy.predict_from_files_sequential([[f]], None)[0], want_seg)
    # with a target: labels in the file's frame, .npz in the RAS frame, .pkl with the reference's keys
    assert toy.predict_from_files(str(src), str(out), save_probabilities=True) == [None]
    labels, linfo = nifti_ref.read(str(out / 's.nii.gz'))
    assert labels.shape == nifti_ref.read(f)[1]['shape'] and labels.shape != want_seg.shape
    assert np.array_equal(orient_ref.apply_zyx(labels, orient_ref.ornt_of(perm, signs)), want_seg)
    assert np.array_equal(_bits32(np.load(out / 's.npz')['probabilities']), _bits32(want_probs))
    pkl = pickle.load(open(out / 's.pkl', 'rb'))
    assert sorted(pkl['nibabel_stuff']) == ['original_affine', 'reoriented_affine'] and pkl['spacing'] == [3.0, 3.0, 3.0]
    assert np.array_equal(pkl['nibabel_stuff']['original_affine'], props['nibabel_stuff']['original_affine'])
    assert np.array_equal(linfo['sform'].astype(np.float32), pkl['nibabel_stuff']['original_affine'].astype(np.float32))
    # predict_single_npy_array with an output file writes the same label file
    assert toy.predict_single_npy_array(img, props, output_file_truncated=str(tmp_path / 'single')) is None
    assert open(tmp_path / 'single.nii.gz', 'rb').read() == open(out / 's.nii.gz', 'rb').read()
    seq = tmp_path / 'seq'
    assert toy.predict_from_files_sequential(str(src), str(seq)) == [None]
    assert open(seq / 's.nii.gz', 'rb').read() == open(out / 's.nii.gz', 'rb').read()


def test_cascade_reads_the_previous_stage_through_the_reorienting_read_seg(tmp_path):
    from fast_nnunet_amd import nnUNetPredictor
    from fast_nnunet_amd.imageio import NiftiReorientIO
    from fast_nnunet_amd.plans import PlansManager
    from golden_cases import toy_unet_spec
    from oracle.unet import synthetic_state_dict
    spec = toy_unet_spec(3, 3)
    cfg = {'patch_size': list(PATCH), 'spacing': [3.0, 3.0, 3.0], 'normalization_schemes': ['ZScoreNormalization'],
           'use_mask_for_norm': [False], 'previous_stage': '3d_lowres',
           'architecture': {'network_class_name': 'PlainConvUNet', 'arch_kwargs': {}, '_kw_requires_import': []}}
    pm = PlansManager({'dataset_name': 'Dataset996_Cascade', 'plans_name': 'nnUNetPlans', 'transpose_forward': [0, 1, 2],
                       'transpose_backward': [0, 1, 2], 'image_reader_writer': 'NibabelIOWithReorient',
                       'foreground_intensity_properties_per_channel': {}, 'configurations': {'3d_fullres': cfg}})
    dj = {'labels': {'background': 0, 'c1': 1, 'c2': 2}, 'channel_names': {'0': 'MR'}, 'file_ending': '.nii.gz'}
    p = nnUNetPredictor(tile_step_size=0.5, use_gaussian=True, use_mirroring=False, device=DEV, allow_tqdm=False,
                        patches_per_forward=3)
    p.manual_initialization(None, pm, pm.get_configuration('3d_fullres'), [synthetic_state_dict(spec, 23)], dj, 'nnUNetTrainer', None)
    assert isinstance(p._reader_writer(), NiftiReorientIO), 'the plans name the class'
    src, prev, out = tmp_path / 'in', tmp_path / 'prev', tmp_path / 'out'
    src.mkdir()
    prev.mkdir()
    perm, signs = ROWS_ORIENTATION
    f = str(src / 'cas_0000.nii.gz')
    _oriented_file(f, _small_ras(31, (18, 22, 40)), 4, perm, signs)
    img, props = NiftiReorientIO().read_images([f], on_device=False)
    seg = np.random.default_rng(8).integers(0, 3, (18, 22, 40)).astype(np.uint8)           # RAS frame
    NiftiReorientIO().write_seg(seg, str(prev / 'cas.nii.gz'), props)                        # stored in the file's frame
    assert nifti_ref.read(str(prev / 'cas.nii.gz'))[1]['shape'] == nifti_ref.read(f)[1]['shape'] != seg.shape
    assert p.predict_from_files(str(src), str(out), folder_with_segs_from_prev_stage=str(prev)) == [None]
    want = p.predict_single_npy_array(img, props, segmentation_previous_stage=seg[None])
    got = orient_ref.apply_zyx(nifti_ref.read(str(out / 'cas.nii.gz'))[0], orient_ref.ornt_of(perm, signs))
    assert np.array_equal(got, want)
    other = p.predict_single_npy_array(img, props, segmentation_previous_stage=np.zeros_like(seg[None]))
    assert (other != want).any(), 'the previous stage reaches the network'


def test_a_failing_case_raises_and_leaves_no_thread_and_no_partial_file(toy, tmp_path):
    src, out = tmp_path / 'in', tmp_path / 'out'
    src.mkdir()
    perm, signs = TRANSPOSE_ORIENTATION
    files = [str(src / f'k{i}_0000.nii.gz') for i in range(3)]
    for i, f in enumerate(files):
        _oriented_file(f, _small_ras(50 + i), 4, perm, signs)
    blob = nifti_ref.file_bytes(files[1])
    with gzip.open(files[1], 'wb') as g:
        g.write(blob[:len(blob) // 2])
    with pytest.raises(RuntimeError, match='k1_0000'):
        toy.predict_from_files(str(src), str(out))
    assert not [t.name for t in threading.enumerate() if t.name.startswith('fnn-')], 'reader and writer threads have ended'
    made = sorted(os.listdir(out))
    assert not [m for m in made if m.startswith('k1') or '.part' in m], made
    labels = nifti_ref.read(str(out / 'k0.nii.gz'))[0]                                       # the case before it was finished, whole
    assert labels.shape == nifti_ref.read(files[0])[1]['shape']
