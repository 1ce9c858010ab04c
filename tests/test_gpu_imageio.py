"""Image files on a real MI355X: ``fnn_decode_voxels`` against numpy bit for bit, ``NiftiIO.read_images`` on the device
against the independent reader tests/nifti_ref.py, and the case pipeline (``predict_from_files``,
``predict_from_files_sequential``, ``predict_single_npy_array(output_file_truncated=...)``) against
``predict_single_npy_array`` fed with nifti_ref's arrays and properties: equal labels, bit-equal probabilities.

Kernels launched here (csrc/imageio.hip): decode_voxels_kernel<unsigned char>, <signed char>, <short>, <unsigned short>,
<int>, <unsigned int>, <float> and <double> - one per NIfTI datatype code of ``DATATYPES`` below, each with and without the
shifted body (``out`` 0..3 elements past a 16-byte boundary), with no body at all (n_vox 1, 3) and with edges on both sides.
"""
import gzip
import os
import pickle
import shutil
import threading
from fractions import Fraction

import numpy as np
import pytest
import torch

import nifti_ref
from golden_cases import toy_unet_spec
from oracle.unet import synthetic_state_dict
from test_gpu_predictor import _toy_model_folder

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda', 0)
CT = 'example_ct_sm.nii.gz'
SEG = 'example_ct_sm_T300_output.nii.gz'
DATATYPES = {2: 'u1', 256: 'i1', 4: 'i2', 512: 'u2', 8: 'i4', 768: 'u4', 16: 'f4', 64: 'f8'}
KERNEL_OF = {2: 'decode_voxels_kernel<unsigned char>', 256: 'decode_voxels_kernel<signed char>',
             4: 'decode_voxels_kernel<short>', 512: 'decode_voxels_kernel<unsigned short>', 8: 'decode_voxels_kernel<int>',
             768: 'decode_voxels_kernel<unsigned int>', 16: 'decode_voxels_kernel<float>', 64: 'decode_voxels_kernel<double>'}
N_VOX = (1, 3, 15, 16, 17, 1029, 30 * 101 * 122)
SENTINEL = np.uint32(0xdeadbeef)


# ---------------------------------------------------------------------------------------------------------------
# fnn_decode_voxels
# ---------------------------------------------------------------------------------------------------------------
def _fused_pair():
    """(slope, inter, v): float64 constants for which (double)v * slope + inter rounded ONCE (what a fused multiply-add
    gives) and rounded TWICE (product, then sum: numpy, and the value rule) end in different float32 values.
    slope = fl(1 / 3) and v = 3: the exact product is 1 - 2^-54, which rounds to 1.0.  With inter = t - 1 the two-step sum is
    exactly t; t is a float32 tie whose even neighbour lies above it, so it rounds up, while the single-rounding sum
    t - 2^-54 lies below the tie and rounds down."""
    v, slope = 3, 1.0 / 3.0
    exact = Fraction(v) * Fraction(slope)
    assert float(exact) == 1.0 and exact != 1
    for k in range(64):
        t = Fraction(2) ** -28 * (1 + Fraction(2 * k + 1, 2 ** 24))           # halfway between two float32 neighbours
        inter = t - 1
        if Fraction(float(inter)) != inter:
            continue
        two_step = np.float32(np.float64(v) * np.float64(slope) + np.float64(float(inter)))
        single = np.float32(float(exact + inter))                              # float(Fraction) rounds correctly, once
        if two_step != single:
            return slope, float(inter), v
    raise AssertionError('no pair found')


def _values(code, n):
    """n values of the datatype, the ones that make the rounding visible first."""
    rng = np.random.default_rng(code)
    dt = np.dtype(DATATYPES[code])
    if dt.kind in 'iu':
        info = np.iinfo(dt)
        special = [3, 0, info.max, info.min, 1, info.max - 1]
        if dt.itemsize == 4:
            # beyond 2^24 a float32 no longer holds every integer: ties (to even, both ways) and their neighbours
            special += [2 ** 24 + 1, 2 ** 24 + 3, 2 ** 24 + 2, 2 ** 25 + 2, 2 ** 25 + 6, 2 ** 30 + 64, 2 ** 30 + 192, 2 ** 30 + 65]
            special += [-(2 ** 24 + 1), -(2 ** 24 + 3), -(2 ** 30 + 64)] if dt.kind == 'i' else \
                       [2 ** 31 + 128, 2 ** 31 + 384, 2 ** 31 + 129, 2 ** 32 - 1, 2 ** 32 - 128, 2 ** 32 - 129]
        body = rng.integers(info.min, int(info.max) + 1, n, dtype=np.int64 if dt.itemsize < 8 else None)
        out = np.concatenate([np.array(special, dtype=np.int64), body])[:n].astype(dt)
        return out
    special = [3.0, np.nan, np.inf, -np.inf, -0.0, 0.0, 1.5, -2.75]
    if code == 64:
        # between float32 neighbours: exact ties both ways, just off a tie, overflow, underflow into the denormals and to 0
        special += [1 + 2.0 ** -24, 1 + 3 * 2.0 ** -24, 1 + 2.0 ** -24 + 2.0 ** -50, 1 + 2.0 ** -24 - 2.0 ** -50,
                    -(1 + 2.0 ** -24), 3.4028235677973366e38, 3.4028235e38, 1e39, -1e39, 2.0 ** -149, 2.0 ** -150,
                    1.5 * 2.0 ** -150, 2.0 ** -127 + 2.0 ** -151, 1e-50, 0.1, 1 / 3]
    else:
        special += [np.float32(1e-40), np.float32(-1e-45), np.float32(3.4028235e38), np.float32(1.17549435e-38)]
    body = rng.standard_normal(n) * 10.0 ** rng.integers(-3, 6, n)
    return np.concatenate([np.array(special, dtype=np.float64), body])[:n].astype(dt)


def _expected(v, scale, slope, inter):
    """The issue's numpy expression np.float32(np.float64(v) * np.float64(slope) + np.float64(inter)) - with the value
    rule's skips spelled out (they only show for -0.0, which an added 0.0 would turn into +0.0) - or the plain cast."""
    with np.errstate(over='ignore', invalid='ignore'):
        if not scale:
            return v.astype(np.float32)
        d = v.astype(np.float64)
        if slope != 1:
            d = d * np.float64(slope)
        if inter != 0:
            d = d + np.float64(inter)
        return d.astype(np.float32)


def _bits32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_the_fused_pair_is_one_where_numpy_and_a_single_rounding_differ():
    slope, inter, v = _fused_pair()
    exact = Fraction(v) * Fraction(slope) + Fraction(inter)
    two_step = np.float32(np.float64(v) * np.float64(slope) + np.float64(inter))
    assert np.float32(float(exact)) != two_step
    assert np.float64(v) * np.float64(slope) + np.float64(inter) != float(exact), 'they differ in float64 already'


@pytest.mark.parametrize('code', sorted(DATATYPES), ids=[KERNEL_OF[c] for c in sorted(DATATYPES)])
def test_decode_voxels_matches_numpy_bit_for_bit(code):
    from fast_nnunet_amd import capi
    f_slope, f_inter, f_v = _fused_pair()
    scalings = [('none', 0, 1.0, 0.0), ('slope', 1, 0.30000001192092896, 0.0), ('inter', 1, 1.0, -1024.5),
                ('both', 1, -2.5, 0.001), ('both_fused_pair', 1, f_slope, f_inter), ('slope_fused', 1, f_slope, 0.0)]
    dt = np.dtype(DATATYPES[code])
    stream = torch.cuda.current_stream(DEV).cuda_stream
    worst = 0
    fused_seen = False
    for n in N_VOX:
        v = _values(code, n)
        for swap in (0, 1):
            raw_host = (v.byteswap() if swap else v).tobytes()
            raw = torch.frombuffer(bytearray(raw_host), dtype=torch.uint8).to(DEV)
            assert raw.data_ptr() % 16 == 0
            for name, scale, slope, inter in scalings:
                want = _expected(v, scale, slope, inter)
                if name == 'both_fused_pair' and n >= 1:
                    single = np.float32(float(Fraction(float(v[0])) * Fraction(slope) + Fraction(inter))) if np.isfinite(float(v[0])) else None
                    assert v[0] == f_v and single is not None and single != want[0]
                    fused_seen = True
                for off in (0, 1, 2, 3):
                    buf = torch.from_numpy(np.full(n + 12, SENTINEL, dtype=np.uint32).view(np.int32).copy()).to(DEV)
                    assert buf.data_ptr() % 16 == 0
                    capi.decode_voxels(raw.data_ptr(), code, swap, n, scale, slope, inter, buf.data_ptr() + 4 * (4 + off), stream)
                    got = buf.cpu().numpy().view(np.uint32)
                    lo = 4 + off
                    assert np.all(got[:lo] == SENTINEL) and np.all(got[lo + n:] == SENTINEL), (n, swap, name, off, 'wrote outside out[0, n_vox)')
                    diff = got[lo:lo + n] != _bits32(want)
                    if diff.any():
                        i = int(np.flatnonzero(diff)[0])
                        raise AssertionError(f'{KERNEL_OF[code]} n_vox={n} byteswap={swap} scaling={name} out offset={off}: element {i} '
                                             f'(value {v[i]!r}) is {got[lo + i]:#010x}, numpy gives {_bits32(want)[i]:#010x}; '
                                             f'{int(diff.sum())} of {n} differ')
                    worst += 1
    assert fused_seen and worst == len(N_VOX) * 2 * len(scalings) * 4
    print(f'{KERNEL_OF[code]} ({dt.name}): {worst} launches bit-identical to numpy')


def test_decode_voxels_refuses_what_it_cannot_serve():
    from fast_nnunet_amd import capi
    raw = torch.zeros(64, dtype=torch.uint8, device=DEV)
    out = torch.full((32,), 7.0, dtype=torch.float32, device=DEV)
    for shift in (1, 2, 4, 8):
        with pytest.raises(AssertionError, match='16-byte'):
            capi.decode_voxels(raw.data_ptr() + shift, 2, 0, 8, 0, 1.0, 0.0, out.data_ptr())
    with pytest.raises(AssertionError):
        capi.decode_voxels(raw.data_ptr(), 2, 0, 8, 0, 1.0, 0.0, out.data_ptr() + 2)
    for code in (0, 1, 32, 128, 1024, 1280, 1536, 1792, 2304, 3):
        with pytest.raises(NotImplementedError):
            capi.decode_voxels(raw.data_ptr(), code, 0, 8, 0, 1.0, 0.0, out.data_ptr())
    with pytest.raises(AssertionError):
        capi.decode_voxels(raw.data_ptr(), 2, 0, -1, 0, 1.0, 0.0, out.data_ptr())
    host = np.zeros(64, np.uint8)
    with pytest.raises(AssertionError, match='device'):
        capi.decode_voxels(host.ctypes.data - host.ctypes.data % 16 + 16, 2, 0, 8, 0, 1.0, 0.0, out.data_ptr())
    capi.decode_voxels(raw.data_ptr(), 2, 0, 0, 0, 1.0, 0.0, out.data_ptr())            # nothing to do
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()), 'a refused or empty call writes nothing'


# ---------------------------------------------------------------------------------------------------------------
# NiftiIO.read_images on the device
# ---------------------------------------------------------------------------------------------------------------
def test_read_images_on_the_device_equals_the_yardstick_on_the_ct_fixture(golden_dir):
    from fast_nnunet_amd.imageio import NiftiIO
    f = os.path.join(golden_dir, CT)
    got, props = NiftiIO(DEV).read_images([f])
    want, info = nifti_ref.read(f)
    assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == (1, 30, 101, 122)
    assert np.array_equal(_bits32(got.cpu().numpy()[0]), _bits32(want))
    assert props['spacing'] == info['spacing'] and np.array_equal(props['nibabel_stuff']['original_affine'], info['affine'])
    host, props_host = NiftiIO().read_images([f], on_device=False)
    assert np.array_equal(_bits32(host), _bits32(got.cpu().numpy())) and props_host['spacing'] == props['spacing']
    seg, _ = NiftiIO(DEV).read_seg(os.path.join(golden_dir, SEG))
    assert np.array_equal(seg.cpu().numpy()[0], nifti_ref.read(os.path.join(golden_dir, SEG))[0])


def _two_channel_case(folder, name='pair', seed=3):
    """9 x 11 x 13 voxels (odd n_vox: the second channel starts 4 bytes off a 16-byte boundary): big-endian float32 and
    uint8 with slope 0.5 and intercept -3."""
    rng = np.random.default_rng(seed)
    a = (rng.standard_normal((9, 11, 13)) * 200).astype(np.float32)
    b = rng.integers(0, 256, (9, 11, 13)).astype(np.uint8)
    a[:2] = 0
    a[3, 0, :4] = [np.float32(-0.0), np.float32(1e-40), 3.0, -7.25]
    b[:2] = 6                                                     # 6 * 0.5 - 3 = 0: the non-zero crop has something to cut
    sform = np.diag([1.5, 1.5, 2.0, 1.0])
    files = [os.path.join(folder, f'{name}_0000.nii.gz'), os.path.join(folder, f'{name}_0001.nii.gz')]
    nifti_ref.write(files[0], a, 16, order='>', sform=sform, sform_code=1, pixdim=(1, 1.5, 1.5, 2.0))
    nifti_ref.write(files[1], b, 2, order='>', slope=0.5, inter=-3.0, sform=sform, sform_code=1, pixdim=(1, 1.5, 1.5, 2.0))
    return files


def test_read_images_of_a_two_file_case_with_an_odd_voxel_count(tmp_path):
    from fast_nnunet_amd.imageio import NiftiIO
    files = _two_channel_case(str(tmp_path))
    got, props = NiftiIO(DEV).read_images(files)
    want = np.stack([nifti_ref.read(f)[0] for f in files])
    assert tuple(got.shape) == (2, 9, 11, 13) and (9 * 11 * 13) % 4 == 3
    assert np.array_equal(_bits32(got.cpu().numpy()), _bits32(want))
    assert np.array_equal(want[1], np.float32(np.float64(nifti_ref.read(files[1])[1]['header']['scl_slope']) *
                                              np.frombuffer(nifti_ref.file_bytes(files[1])[352:], np.uint8).reshape(9, 11, 13) - 3.0))
    assert props['spacing'] == [2.0, 1.5, 1.5]
    # refusals come before anything is uploaded or launched: a truncated second file leaves the device untouched
    blob = nifti_ref.file_bytes(files[1])
    with gzip.open(files[1], 'wb') as f:
        f.write(blob[:-5])
    before = torch.cuda.memory_allocated(DEV)
    with pytest.raises(RuntimeError, match='pair_0001'):
        NiftiIO(DEV).read_images(files)
    assert torch.cuda.memory_allocated(DEV) == before


# ---------------------------------------------------------------------------------------------------------------
# the case pipeline
# ---------------------------------------------------------------------------------------------------------------
PATCH = (16, 16, 32)


@pytest.fixture(scope='module')
def toy(tmp_path_factory):
    """One toy model folder (1 channel, 3 classes, plans at 3 mm: the CT fixture's spacing) and its predictor."""
    from fast_nnunet_amd import nnUNetPredictor
    folder, plans, dj, sd, spec = _toy_model_folder(tmp_path_factory.mktemp('toy'), PATCH, 3, plans_spacing=(3.0, 3.0, 3.0))
    p = nnUNetPredictor(tile_step_size=0.5, use_gaussian=True, use_mirroring=False, device=DEV, allow_tqdm=False,
                        patches_per_forward=4)
    p.initialize_from_trained_model_folder(str(folder), use_folds=(0,))
    return p


def _manual_predictor(in_channels, heads=3, previous_stage=None, image_channels=None):
    """A predictor of a network with `in_channels` inputs (two images, or an image and the one-hot previous stage)."""
    from fast_nnunet_amd import nnUNetPredictor
    from fast_nnunet_amd.plans import PlansManager
    image_channels = image_channels or in_channels
    spec = toy_unet_spec(in_channels, heads)
    cfg = {'patch_size': list(PATCH), 'spacing': [2.0, 1.5, 1.5], 'normalization_schemes': ['ZScoreNormalization'] * image_channels,
           'use_mask_for_norm': [False] * image_channels,
           'architecture': {'network_class_name': 'PlainConvUNet', 'arch_kwargs': {}, '_kw_requires_import': []}}
    if previous_stage:
        cfg['previous_stage'] = previous_stage
    pm = PlansManager({'dataset_name': 'Dataset998_Files', 'plans_name': 'nnUNetPlans', 'transpose_forward': [0, 1, 2],
                       'transpose_backward': [0, 1, 2], 'image_reader_writer': 'NibabelIO',
                       'foreground_intensity_properties_per_channel': {}, 'configurations': {'3d_fullres': cfg}})
    dj = {'labels': {('background' if i == 0 else f'c{i}'): i for i in range(heads)},
          'channel_names': {str(i): 'MR' for i in range(image_channels)}, 'file_ending': '.nii.gz'}
    p = nnUNetPredictor(tile_step_size=0.5, use_gaussian=True, use_mirroring=False, device=DEV, allow_tqdm=False,
                        patches_per_forward=3)
    p.manual_initialization(None, pm, pm.get_configuration('3d_fullres'), [synthetic_state_dict(spec, 23)], dj, 'nnUNetTrainer', None)
    return p


def _ref_case(files):
    """What a caller of predict_single_npy_array holds after reading the files with the yardstick."""
    reads = [nifti_ref.read(f) for f in files]
    return np.stack([r[0] for r in reads]), nifti_ref.properties(reads[0][1])


def _small_case(folder, name, seed, shape=(18, 20, 36), spacing=(3.0, 3.0, 3.0)):
    """One int16 file <name>_0000.nii.gz with a zero border; spacing in (z, y, x)."""
    rng = np.random.default_rng(seed)
    v = (rng.standard_normal(shape) * 300 + 100).astype(np.int16)
    v[:2] = 0
    v[:, :, -3:] = 0
    sform = np.diag([spacing[2], spacing[1], spacing[0], 1.0])
    sform[:3, 3] = [-10.0, 20.5, 3.0]
    f = os.path.join(folder, f'{name}_0000.nii.gz')
    nifti_ref.write(f, v, 4, sform=sform, sform_code=2, pixdim=(1, spacing[2], spacing[1], spacing[0]))
    return f


def _read_labels(f):
    values, info = nifti_ref.read(f)
    return values, info


def test_ct_fixture_through_the_folder_form(toy, tmp_path, golden_dir):
    src, out = tmp_path / 'in', tmp_path / 'out'
    src.mkdir()
    shutil.copy(os.path.join(golden_dir, CT), src / 'ct_0000.nii.gz')
    ret = toy.predict_from_files(str(src), str(out), num_processes_preprocessing=2, num_processes_segmentation_export=2)
    assert ret == [None]
    img, props = _ref_case([str(src / 'ct_0000.nii.gz')])
    want = toy.predict_single_npy_array(img, props)
    got, info = _read_labels(str(out / 'ct.nii.gz'))
    assert want.dtype == np.uint8 and len(np.unique(want)) >= 2
    assert np.array_equal(got, want)
    # the geometry of the input, in the header the reference's own output fixture has
    assert nifti_ref.file_bytes(str(out / 'ct.nii.gz'))[:352] == nifti_ref.file_bytes(os.path.join(golden_dir, SEG))[:352]
    assert sorted(os.listdir(out)) == ['ct.nii.gz', 'dataset.json', 'plans.json', 'predict_from_raw_data_args.json']
    import json
    assert json.load(open(out / 'dataset.json')) == toy.dataset_json and json.load(open(out / 'plans.json')) == toy.plans_manager.plans
    args = json.load(open(out / 'predict_from_raw_data_args.json'))
    assert args['list_of_lists_or_source_folder'] == str(src) and args['overwrite'] is True and args['num_parts'] == 1


def test_resampled_case_with_probabilities_npz_pkl_and_labels(toy, tmp_path):
    src, out = tmp_path / 'in', tmp_path / 'out'
    src.mkdir()
    f = _small_case(str(src), 'fine', 4, shape=(20, 26, 44), spacing=(2.0, 2.5, 2.0))          # plans: 3 mm -> resampled
    assert toy.predict_from_files(str(src), str(out), save_probabilities=True) == [None]
    img, props = _ref_case([f])
    want_seg, want_probs = toy.predict_single_npy_array(img, props, save_or_return_probabilities=True)
    assert np.array_equal(_read_labels(str(out / 'fine.nii.gz'))[0], want_seg)
    with np.load(out / 'fine.npz') as z:
        assert list(z.keys()) == ['probabilities']
        probs = z['probabilities']
    assert probs.dtype == np.float32 and np.array_equal(_bits32(probs), _bits32(want_probs))
    pkl = pickle.load(open(out / 'fine.pkl', 'rb'))
    assert pkl['spacing'] == [2.0, 2.5, 2.0] and np.array_equal(pkl['nibabel_stuff']['original_affine'], props['nibabel_stuff']['original_affine'])
    assert tuple(pkl['shape_before_cropping']) == (20, 26, 44)
    assert [list(b) for b in pkl['bbox_used_for_cropping']] == [[2, 20], [0, 26], [0, 41]]
    assert tuple(pkl['shape_after_cropping_and_before_resampling']) == (18, 26, 41)
    # the written label file carries the pickled geometry
    assert np.array_equal(_read_labels(str(out / 'fine.nii.gz'))[1]['affine'], pkl['nibabel_stuff']['original_affine'])


def test_two_channel_case_and_results_returned_without_an_output_target(tmp_path):
    p = _manual_predictor(2)
    files = _two_channel_case(str(tmp_path))
    img, props = _ref_case(files)
    want_seg, want_probs = p.predict_single_npy_array(img, props, save_or_return_probabilities=True)
    ret = p.predict_from_files([files], None, save_probabilities=True)
    assert len(ret) == 1 and np.array_equal(ret[0][0], want_seg) and np.array_equal(_bits32(ret[0][1]), _bits32(want_probs))
    ret = p.predict_from_files_sequential([files], None)
    assert len(ret) == 1 and np.array_equal(ret[0], p.predict_single_npy_array(img, props))
    assert sorted(os.listdir(tmp_path)) == ['pair_0000.nii.gz', 'pair_0001.nii.gz'], 'nothing is written without a target'
    # the list form with truncated output names
    out = tmp_path / 'o'
    assert p.predict_from_files([files], [str(out / 'first')]) == [None]
    assert np.array_equal(_read_labels(str(out / 'first.nii.gz'))[0], ret[0])
    assert p.predict_from_files([], [], save_probabilities=True) is None and p.predict_from_files_sequential([], None) is None


def test_overwrite_false_num_parts_and_the_sequential_form(toy, tmp_path):
    src, out, seq = tmp_path / 'in', tmp_path / 'out', tmp_path / 'seq'
    src.mkdir()
    files = [_small_case(str(src), f'c{i}', 10 + i, shape=(17 + i, 20, 34 + i)) for i in range(4)]
    want = []
    for f in files:
        img, props = _ref_case([f])
        want.append(toy.predict_single_npy_array(img, props))
    # two parts of the folder: disjoint, together everything
    assert toy.predict_from_files(str(src), str(out), num_parts=2, part_id=0) == [None, None]
    assert sorted(i for i in os.listdir(out) if i.endswith('.nii.gz')) == ['c0.nii.gz', 'c2.nii.gz']
    assert toy.predict_from_files(str(src), str(out), num_parts=2, part_id=1) == [None, None]
    for i in range(4):
        assert np.array_equal(_read_labels(str(out / f'c{i}.nii.gz'))[0], want[i]), i
    # overwrite=False: only what is missing is made again
    os.remove(out / 'c1.nii.gz')
    stamps = {i: os.stat(out / f'c{i}.nii.gz').st_mtime_ns for i in (0, 2, 3)}
    for i in (0, 2, 3):
        os.utime(out / f'c{i}.nii.gz', ns=(1, 1))
    assert toy.predict_from_files(str(src), str(out), overwrite=False) == [None]
    assert all(os.stat(out / f'c{i}.nii.gz').st_mtime_ns == 1 for i in stamps), 'existing outputs were left alone'
    assert np.array_equal(_read_labels(str(out / 'c1.nii.gz'))[0], want[1])
    assert toy.predict_from_files(str(src), str(out), overwrite=False) is None                 # nothing left to do
    # with probabilities asked for, a label file without its .npz does not count as done
    assert toy.predict_from_files(str(src), str(out), overwrite=False, save_probabilities=True, num_parts=4, part_id=3) == [None]
    assert os.path.isfile(out / 'c3.npz') and os.path.isfile(out / 'c3.pkl') and os.stat(out / 'c3.nii.gz').st_mtime_ns != 1
    # the sequential form and the threaded one write the same files
    assert toy.predict_from_files_sequential(str(src), str(seq)) == [None] * 4
    for i in range(4):
        assert open(seq / f'c{i}.nii.gz', 'rb').read() == open(out / f'c{i}.nii.gz', 'rb').read(), i
    inline = tmp_path / 'inline'
    assert toy.predict_from_files(str(src), str(inline), num_processes_preprocessing=0, num_processes_segmentation_export=0) == [None] * 4
    assert all(open(inline / f'c{i}.nii.gz', 'rb').read() == open(seq / f'c{i}.nii.gz', 'rb').read() for i in range(4))
    assert not [t.name for t in threading.enumerate() if t.name.startswith('fnn-')]


def test_cascade_reads_the_previous_stage_with_read_seg(tmp_path):
    p = _manual_predictor(3, heads=3, previous_stage='3d_lowres', image_channels=1)
    src, prev, out = tmp_path / 'in', tmp_path / 'prev', tmp_path / 'out'
    src.mkdir()
    prev.mkdir()
    f = _small_case(str(src), 'cas', 31, shape=(18, 22, 40), spacing=(2.0, 1.5, 1.5))
    seg = np.random.default_rng(8).integers(0, 3, (18, 22, 40)).astype(np.uint8)
    from fast_nnunet_amd.imageio import write_nifti_seg
    img, props = _ref_case([f])
    write_nifti_seg(seg, str(prev / 'cas.nii.gz'), props)
    with pytest.raises(AssertionError, match='cascaded'):
        p.predict_from_files(str(src), str(out))
    assert p.predict_from_files(str(src), str(out), folder_with_segs_from_prev_stage=str(prev)) == [None]
    seg_ref = nifti_ref.read(str(prev / 'cas.nii.gz'))[0][None]
    want = p.predict_single_npy_array(img, props, segmentation_previous_stage=seg_ref)
    assert np.array_equal(_read_labels(str(out / 'cas.nii.gz'))[0], want)
    other = p.predict_single_npy_array(img, props, segmentation_previous_stage=np.zeros_like(seg_ref))
    assert (other != want).any(), 'the previous stage reaches the network'
    assert np.array_equal(p.predict_from_files_sequential(str(src), None, folder_with_segs_from_prev_stage=str(prev))[0], want)


def _swap_labels(segmentation, a, b):
    """A postprocessing step of the caller's own: labels a and b exchanged."""
    out = segmentation.copy()
    out[segmentation == a] = b
    out[segmentation == b] = a
    return out


def test_single_array_export_and_postprocessing_before_the_write(toy, tmp_path):
    f = _small_case(str(tmp_path), 'one', 41)
    img, props = _ref_case([f])
    want = toy.predict_single_npy_array(img, props)
    assert toy.predict_single_npy_array(img, props, output_file_truncated=str(tmp_path / 'exported')) is None
    assert np.array_equal(_read_labels(str(tmp_path / 'exported.nii.gz'))[0], want)
    assert not os.path.exists(tmp_path / 'exported.npz')
    assert toy.predict_single_npy_array(img, props, output_file_truncated=str(tmp_path / 'with_probs'),
                                        save_or_return_probabilities=True) is None
    _, want_probs = toy.predict_single_npy_array(img, props, save_or_return_probabilities=True)
    assert np.array_equal(_bits32(np.load(tmp_path / 'with_probs.npz')['probabilities']), _bits32(want_probs))
    assert pickle.load(open(tmp_path / 'with_probs.pkl', 'rb'))['spacing'] == props['spacing']
    # postprocessing set on the predictor is applied before the file is written
    from fast_nnunet_amd.postprocessing import remove_all_but_largest_component_from_segmentation as keep
    # the component step may find nothing to remove in this case's labels; the swap of labels 1 and 2 behind it always shows
    toy.set_postprocessing(([keep, _swap_labels], [{'labels_or_regions': [1, 2]}, {'a': 1, 'b': 2}]))
    try:
        want_pp = toy.predict_single_npy_array(img, props)
        src = tmp_path / 'in'
        src.mkdir()
        shutil.copy(f, src / 'one_0000.nii.gz')
        toy.predict_from_files(str(src), str(tmp_path / 'pp'))
    finally:
        toy.set_postprocessing(None)
    assert np.isin(want, (1, 2)).any() and (want_pp != want).any() and np.array_equal(_read_labels(str(tmp_path / 'pp' / 'one.nii.gz'))[0], want_pp)


def test_a_failing_case_raises_and_leaves_no_thread_and_no_partial_file(toy, tmp_path):
    src, out = tmp_path / 'in', tmp_path / 'out'
    src.mkdir()
    files = [_small_case(str(src), f'k{i}', 50 + i) for i in range(3)]
    blob = nifti_ref.file_bytes(files[1])
    with gzip.open(files[1], 'wb') as f:
        f.write(blob[:len(blob) // 2])
    with pytest.raises(RuntimeError, match='k1_0000'):
        toy.predict_from_files(str(src), str(out), save_probabilities=True)
    assert not [t.name for t in threading.enumerate() if t.name.startswith('fnn-')], 'reader and writer threads have ended'
    made = sorted(os.listdir(out))
    assert not [m for m in made if m.startswith('k1') or '.part' in m], made
    # the case before it was finished, whole
    img, props = _ref_case([files[0]])
    assert np.array_equal(_read_labels(str(out / 'k0.nii.gz'))[0], toy.predict_single_npy_array(img, props))
    assert 'probabilities' in np.load(out / 'k0.npz')
