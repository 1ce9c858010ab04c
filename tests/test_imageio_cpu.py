"""The image reader-writer and the file lists without a GPU: header parsing and its refusals, the scaling rules, the
writer's header against the reference's own output fixture, and the file-list management against what the reference
returned (tests/golden/imageio.json, made by make_golden_imageio.py).  The yardstick for values and geometry is
tests/nifti_ref.py, which shares no code with fast_nnunet_amd.imageio; ``read_images(..., on_device=False)`` is the numpy
route of the reader (the device route is tests/test_gpu_imageio.py)."""
import gzip
import json
import os
import types
import warnings

import numpy as np
import pytest

import nifti_ref

CT = 'example_ct_sm.nii.gz'
SEG = 'example_ct_sm_T300_output.nii.gz'


@pytest.fixture(scope='module')
def io():
    from fast_nnunet_amd import imageio
    return imageio


def _rotation(deg_z=25.0, deg_x=-40.0):
    a, b = np.deg2rad(deg_z), np.deg2rad(deg_x)
    rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
    return rz @ rx


def _volume(shape=(5, 6, 7), seed=0):
    return np.random.default_rng(seed).integers(-1000, 1000, shape).astype(np.int16)


# ---------------------------------------------------------------------------------------------- the fixtures themselves
def test_the_two_fixtures_differ_only_in_datatype_and_bitpix(golden_dir):
    a = gzip.open(os.path.join(golden_dir, CT)).read()
    b = gzip.open(os.path.join(golden_dir, SEG)).read()
    assert [i for i in range(352) if a[i] != b[i]] == [70, 72]
    v, info = nifti_ref.read(os.path.join(golden_dir, CT))
    s, sinfo = nifti_ref.read(os.path.join(golden_dir, SEG))
    assert v.shape == s.shape == (30, 101, 122) and info['spacing'] == [3.0, 3.0, 3.0]
    assert int(info['header']['datatype']) == 4 and int(sinfo['header']['datatype']) == 2
    assert int(info['header']['sform_code']) == 2 and int(info['header']['qform_code']) == 0
    assert sorted(np.unique(s)) == [0.0, 1.0]


def test_fixture_read_on_the_host_equals_the_yardstick(io, golden_dir):
    got, props = io.NiftiIO().read_images([os.path.join(golden_dir, CT)], on_device=False)
    want, info = nifti_ref.read(os.path.join(golden_dir, CT))
    assert got.dtype == np.float32 and got.shape == (1, 30, 101, 122)
    assert np.array_equal(got[0].view(np.uint32), want.view(np.uint32))
    assert props['spacing'] == info['spacing'] and all(type(i) is float for i in props['spacing'])
    aff = props['nibabel_stuff']['original_affine']
    assert aff.dtype == np.float64 and aff.shape == (4, 4) and np.array_equal(aff, info['affine'])
    # the same geometry in ITK's LPS convention: x and y flipped
    sitk = props['sitk_stuff']
    assert sitk['spacing'] == (3.0, 3.0, 3.0)
    assert np.allclose(sitk['origin'], [-aff[0, 3], -aff[1, 3], aff[2, 3]])
    assert np.allclose(np.array(sitk['direction']).reshape(3, 3), np.diag([-1.0, -1.0, 1.0]))
    assert np.array_equal(io.affine_from_sitk_stuff(sitk), aff)
    seg, _ = io.NiftiIO().read_seg(os.path.join(golden_dir, SEG), on_device=False)
    assert np.array_equal(seg[0], nifti_ref.read(os.path.join(golden_dir, SEG))[0])


# ---------------------------------------------------------------------------------------------- header parsing
@pytest.mark.parametrize('order', ['<', '>'])
@pytest.mark.parametrize('ending', ['.nii', '.nii.gz'])
def test_the_three_affine_choices_and_spacing_in_both_byte_orders(io, tmp_path, order, ending):
    vol = _volume()
    rot = _rotation()
    zooms = np.array([0.75, 1.5, 2.25])
    sform = np.eye(4)
    sform[:3, :3] = (rot * zooms).astype(np.float32)
    sform[:3, 3] = np.array([-12.5, 33.25, 7.125], dtype=np.float32)
    # a unit quaternion of another rotation, qfac -1
    q = np.array([0.5, 0.1, -0.3], dtype=np.float32)
    kw = dict(order=order, sform=sform, quatern=tuple(q), qoffset=(4.0, -5.0, 6.5), pixdim=(-1.0, *zooms))
    reader = io.NiftiIO()
    for name, codes in (('sform', dict(sform_code=1, qform_code=1)), ('qform', dict(sform_code=0, qform_code=2)),
                        ('base', dict(sform_code=0, qform_code=0))):
        f = str(tmp_path / f'{name}{ending}')
        nifti_ref.write(f, vol, 4, **kw, **codes)
        got, props = reader.read_images([f], on_device=False)
        want, info = nifti_ref.read(f)
        assert np.array_equal(got[0], want) and got.shape == (1, 5, 6, 7)
        aff = props['nibabel_stuff']['original_affine']
        assert np.allclose(aff, info['affine'], rtol=0, atol=1e-12), name
        assert props['spacing'] == [2.25, 1.5, 0.75] == info['spacing']
        if name == 'sform':
            assert np.array_equal(aff, sform)
        elif name == 'qform':
            # written down here from the NIfTI-1 formula: a = sqrt(1 - b^2 - c^2 - d^2), third column times qfac = -1
            b, c, d = (float(i) for i in q)
            a = np.sqrt(1 - b * b - c * c - d * d)
            r = np.array([[a * a + b * b - c * c - d * d, 2 * b * c - 2 * a * d, 2 * b * d + 2 * a * c],
                          [2 * b * c + 2 * a * d, a * a + c * c - b * b - d * d, 2 * c * d - 2 * a * b],
                          [2 * b * d - 2 * a * c, 2 * c * d + 2 * a * b, a * a + d * d - c * c - b * b]])
            assert np.allclose(aff[:3, :3], r * (zooms * [1, 1, -1]), atol=1e-12)
            assert np.array_equal(aff[:3, 3], [4.0, -5.0, 6.5])
            assert abs(np.linalg.det(aff[:3, :3] / zooms) + 1) < 1e-6          # left-handed: qfac was honoured
        else:
            # zooms on the diagonal (x flipped), the centre voxel (3, 2.5, 2) at the origin
            assert np.array_equal(aff, [[-0.75, 0, 0, 0.75 * 3], [0, 1.5, 0, -1.5 * 2.5], [0, 0, 2.25, -2.25 * 2], [0, 0, 0, 1]])


def _expect_refusal(io, fname, exc=RuntimeError):
    with pytest.raises(exc) as e:
        io.NiftiIO().read_images([fname], on_device=False)
    assert os.path.basename(fname) in str(e.value), 'the message names the file'
    # what the device route runs before it uploads or launches anything refuses the file as well
    with pytest.raises(exc) as e:
        h = io.read_header(fname)
        io.read_voxel_bytes(fname, h, np.empty(h.n_bytes, np.uint8))
    assert os.path.basename(fname) in str(e.value)


@pytest.mark.parametrize('ending', ['.nii', '.nii.gz'])
def test_header_refusals(io, tmp_path, ending):
    vol = _volume()
    f = lambda name: str(tmp_path / (name + ending))            # noqa: E731
    blob = nifti_ref.write(f('ok'), vol, 4)
    io.NiftiIO().read_images([f('ok')], on_device=False)
    # the data end before the header says they do
    opener = gzip.open if ending == '.nii.gz' else open
    with opener(f('truncated'), 'wb') as out:
        out.write(blob[:-3])
    _expect_refusal(io, f('truncated'))
    with opener(f('header_only'), 'wb') as out:
        out.write(blob[:352])
    _expect_refusal(io, f('header_only'))
    with opener(f('short_header'), 'wb') as out:
        out.write(blob[:200])
    _expect_refusal(io, f('short_header'))
    nifti_ref.write(f('four_d'), vol, 4, dim0=4)
    _expect_refusal(io, f('four_d'))
    nifti_ref.write(f('two_d'), vol, 4, dim0=2)
    _expect_refusal(io, f('two_d'))
    nifti_ref.write(f('zero_extent'), vol[:, :, :0], 4)
    _expect_refusal(io, f('zero_extent'))
    nifti_ref.write(f('offset_348'), vol, 4, vox_offset=348)
    _expect_refusal(io, f('offset_348'))
    nifti_ref.write(f('bitpix'), vol, 4, bitpix=32)
    _expect_refusal(io, f('bitpix'))
    for code in (32, 128, 1024, 1280, 1792, 2304, 3):          # complex, RGB, 64-bit integers, RGBA, no datatype at all
        nifti_ref.write(f(f'datatype_{code}'), vol, code, bitpix={32: 64, 128: 24, 1024: 64, 1280: 64, 1792: 128, 2304: 32, 3: 8}[code])
        _expect_refusal(io, f(f'datatype_{code}'))
    # a header that promises more voxels than the file holds (the extent edited after writing)
    big = bytearray(blob)
    big[42:44] = (7000).to_bytes(2, 'little')
    with opener(f('promises_more'), 'wb') as out:
        out.write(bytes(big))
    _expect_refusal(io, f('promises_more'))
    # a later vox_offset needs the bytes too
    nifti_ref.write(f('padded'), vol, 4, vox_offset=400)
    got, _ = io.NiftiIO().read_images([f('padded')], on_device=False)
    assert np.array_equal(got[0], vol)
    late = bytearray(nifti_ref.write(f('tmp'), vol, 4))
    late[108:112] = np.float32(400).tobytes()
    with opener(f('late_offset'), 'wb') as out:
        out.write(bytes(late))
    _expect_refusal(io, f('late_offset'))


def test_other_formats_and_reader_classes_are_refused_by_name(io, tmp_path):
    for name in ('a.nrrd', 'a.mha', 'a.tif', 'a.png', 'a.hdr', 'a.img', 'a.txt'):
        with pytest.raises(NotImplementedError):
            io.NiftiIO().read_images([str(tmp_path / name)], on_device=False)
        with pytest.raises(NotImplementedError):
            io.write_nifti_seg(np.zeros((2, 2, 2), np.uint8), str(tmp_path / name), {'nibabel_stuff': {'original_affine': np.eye(4)}})
    # NIfTI-2 and the two-file form
    vol = _volume()
    blob = bytearray(nifti_ref.write(str(tmp_path / 'x.nii'), vol, 4))
    pair = bytearray(blob)
    pair[344:348] = b'ni1\0'
    (tmp_path / 'pair.nii').write_bytes(bytes(pair))
    with pytest.raises(NotImplementedError):
        io.NiftiIO().read_images([str(tmp_path / 'pair.nii')], on_device=False)
    two = bytearray(blob)
    two[0:4] = (540).to_bytes(4, 'little')
    (tmp_path / 'nifti2.nii').write_bytes(bytes(two))
    with pytest.raises(NotImplementedError):
        io.NiftiIO().read_images([str(tmp_path / 'nifti2.nii')], on_device=False)

    from fast_nnunet_amd.plans import PlansManager
    for name in ('NibabelIO', 'SimpleITKIO'):
        assert PlansManager({'image_reader_writer': name}).image_reader_writer_class is io.NiftiIO
    for name in ('NibabelIOWithReorient', 'SimpleITKIOWithReorient', 'Tiff3DIO', 'NaturalImage2DIO', 'SomethingElseIO'):
        with pytest.raises(NotImplementedError) as e:
            PlansManager({'image_reader_writer': name}).image_reader_writer_class
        assert name in str(e.value)
    assert io.determine_reader_writer_from_dataset_json({'file_ending': '.nii.gz'}) is io.NiftiIO
    assert io.determine_reader_writer_from_dataset_json({'file_ending': '.nii'}) is io.NiftiIO
    assert io.determine_reader_writer_from_dataset_json({'file_ending': '.nii.gz', 'overwrite_image_reader_writer': 'SimpleITKIO'}) is io.NiftiIO
    for dj in ({'file_ending': '.png'}, {'file_ending': '.tif'}, {'file_ending': '.nii.gz', 'overwrite_image_reader_writer': 'NibabelIOWithReorient'}):
        with pytest.raises(NotImplementedError):
            io.determine_reader_writer_from_dataset_json(dj)


def test_files_of_one_case_must_agree_in_shape_and_spacing_but_not_in_affine(io, tmp_path):
    a, b = str(tmp_path / 'a_0000.nii.gz'), str(tmp_path / 'a_0001.nii.gz')
    nifti_ref.write(a, _volume(), 4, pixdim=(1, 1, 2, 3))
    nifti_ref.write(b, _volume((5, 6, 8)), 4, pixdim=(1, 1, 2, 3))
    with pytest.raises(RuntimeError, match='shape'):
        io.NiftiIO().read_images([a, b], on_device=False)
    nifti_ref.write(b, _volume(seed=1), 4, pixdim=(1, 1, 2, 3.5))
    with pytest.raises(RuntimeError, match='spacing'):
        io.NiftiIO().read_images([a, b], on_device=False)
    # another origin: a warning, and the first file's affine
    s0, s1 = np.eye(4), np.eye(4)
    s1[:3, 3] = [1, 2, 3]
    nifti_ref.write(a, _volume(), 4, pixdim=(1, 1, 2, 3), sform=s0, sform_code=1)
    nifti_ref.write(b, _volume(seed=1), 16, pixdim=(1, 1, 2, 3), sform=s1, sform_code=1)
    with pytest.warns(UserWarning, match='affine'):
        got, props = io.NiftiIO().read_images([a, b], on_device=False)
    assert got.shape == (2, 5, 6, 7) and np.array_equal(props['nibabel_stuff']['original_affine'], s0)
    assert np.array_equal(got[0], _volume()) and np.array_equal(got[1], _volume(seed=1))
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        io.NiftiIO().read_images([a, a], on_device=False)


# ---------------------------------------------------------------------------------------------- scaling
def test_scaling_follows_get_slope_inter(io, tmp_path):
    vol = _volume()
    f = str(tmp_path / 's.nii')
    for slope, inter in ((0.0, 5.0), (np.nan, 5.0), (np.inf, 1.0), (-np.inf, np.nan), (1.0, 0.0)):     # no scaling at all
        nifti_ref.write(f, vol, 4, slope=slope, inter=inter)
        h = io.read_header(f)
        assert not h.scale and (h.slope, h.inter) == (1.0, 0.0)
        assert np.array_equal(io.NiftiIO().read_images([f], on_device=False)[0][0], vol)
    for inter in (np.nan, np.inf):
        nifti_ref.write(f, vol, 4, slope=2.0, inter=inter)
        with pytest.raises(RuntimeError, match='s.nii'):
            io.NiftiIO().read_images([f], on_device=False)
    for slope, inter in ((0.1, 0.0), (1.0, -1024.0), (0.30000001192092896, 7.7), (-2.5, 1e-3)):
        nifti_ref.write(f, vol, 4, slope=slope, inter=inter)
        h = io.read_header(f)
        assert h.scale and h.slope == float(np.float32(slope)) and h.inter == float(np.float32(inter))
        got = io.NiftiIO().read_images([f], on_device=False)[0][0]
        want = np.float32(np.float64(vol) * np.float64(np.float32(slope)) + np.float64(np.float32(inter)))
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
        assert np.array_equal(got.view(np.uint32), nifti_ref.read(f)[0].view(np.uint32))


@pytest.mark.parametrize('code', sorted(nifti_ref.NUMPY_TYPES))
@pytest.mark.parametrize('order', ['<', '>'])
def test_every_datatype_on_the_host_route(io, tmp_path, code, order):
    rng = np.random.default_rng(code)
    vol = (rng.standard_normal((3, 4, 5)) * 1e5) if code in (16, 64) else rng.integers(-2 ** 31, 2 ** 32, (3, 4, 5))
    f = str(tmp_path / 'd.nii.gz')
    nifti_ref.write(f, vol, code, order=order, slope=0.5, inter=-3.0)
    got = io.NiftiIO().read_images([f], on_device=False)[0][0]
    assert np.array_equal(got.view(np.uint32), nifti_ref.read(f)[0].view(np.uint32))


# ---------------------------------------------------------------------------------------------- writing
def test_written_header_equals_the_references_output_fixture_byte_for_byte(io, tmp_path, golden_dir):
    reader = io.NiftiIO()
    _, props = reader.read_images([os.path.join(golden_dir, CT)], on_device=False)
    labels, _ = reader.read_seg(os.path.join(golden_dir, SEG), on_device=False)
    fixture = gzip.open(os.path.join(golden_dir, SEG)).read()
    for name in ('out.nii.gz', 'out.nii'):
        f = str(tmp_path / name)
        reader.write_seg(labels[0], f, props)
        made = nifti_ref.file_bytes(f)
        assert made[:352] == fixture[:352]
        assert made[352:] == fixture[352:] and len(made) == 352 + 30 * 101 * 122
    assert sorted(os.listdir(tmp_path)) == ['out.nii', 'out.nii.gz'], 'no temporary file is left'
    raw = open(tmp_path / 'out.nii.gz', 'rb').read()
    assert raw[:2] == b'\x1f\x8b' and raw[8] == 4, 'gzip, fastest level'
    # and from the ITK statement of the same geometry alone
    reader.write_seg(labels[0], str(tmp_path / 'sitk.nii'), {'sitk_stuff': props['sitk_stuff'], 'spacing': props['spacing']})
    assert nifti_ref.file_bytes(str(tmp_path / 'sitk.nii')) == fixture


def test_label_dtype_rule_and_round_trip(io, tmp_path):
    rng = np.random.default_rng(5)
    props = {'nibabel_stuff': {'original_affine': np.diag([2.0, 2.0, 4.0, 1.0])}}
    for top, code in ((254, 2), (255, 512), (3000, 512), (0, 2)):
        seg = rng.integers(0, top + 1, (4, 5, 6))
        seg[0, 0, 0] = top
        for dtype in (np.uint8 if top < 256 else np.uint16, np.int64):
            f = str(tmp_path / f'seg_{top}.nii.gz')
            io.write_nifti_seg(seg.astype(dtype), f, props)
            got, info = nifti_ref.read(f)
            assert int(info['header']['datatype']) == code and int(info['header']['bitpix']) == (16 if code == 512 else 8)
            assert np.array_equal(got, seg) and info['spacing'] == [4.0, 2.0, 2.0]
            back, p2 = io.NiftiIO().read_seg(f, on_device=False)
            assert np.array_equal(back[0], seg) and np.array_equal(p2['nibabel_stuff']['original_affine'], info['affine'])


def test_a_rotated_affine_survives_through_sform_and_qform(io, tmp_path):
    aff = np.eye(4)
    zooms = np.array([0.8, 0.8, 2.5])
    aff[:3, :3] = (_rotation(33.0, 12.0) * zooms).astype(np.float32)
    aff[:3, 3] = np.array([-101.5, 57.25, -3.0], dtype=np.float32)
    mirrored = aff.copy()
    mirrored[:3, 2] *= -1                                       # left-handed: qfac = -1
    for n, a in enumerate((aff, mirrored)):
        f = str(tmp_path / f'rot{n}.nii')
        io.write_nifti_seg(np.ones((3, 4, 5), np.uint8), f, {'nibabel_stuff': {'original_affine': a}})
        _, info = nifti_ref.read(f)
        h = info['header']
        assert int(h['sform_code']) == 2 and int(h['qform_code']) == 0
        assert np.array_equal(info['sform'], a), 'the sform holds the float32 affine exactly'
        assert float(h['pixdim'][0]) == (1.0 if n == 0 else -1.0)
        assert np.abs(info['qform'] - a).max() < 1e-6
        assert np.allclose(h['pixdim'][1:4], zooms, atol=1e-6)
        # our own reader takes the sform
        assert np.array_equal(io.read_header(f).affine, a)


# ---------------------------------------------------------------------------------------------- file lists
def _golden(golden_dir):
    return json.load(open(os.path.join(golden_dir, 'imageio.json')))


def _put(obj, root):
    if isinstance(obj, str):
        return obj.replace('<root>', root)
    if isinstance(obj, list):
        return [_put(i, root) for i in obj]
    return obj


def _make_folders(doc, root):
    for name, files in doc['folders'].items():
        os.makedirs(os.path.join(root, name), exist_ok=True)
        for f in files:
            open(os.path.join(root, name, f), 'w').close()


def test_lists_of_a_source_folder_equal_the_references(golden_dir, tmp_path):
    from fast_nnunet_amd.predictor import create_lists_from_splitted_dataset_folder
    doc, root = _golden(golden_dir), str(tmp_path)
    _make_folders(doc, root)
    assert len(doc['lists']) >= 6
    for case in doc['lists']:
        got = create_lists_from_splitted_dataset_folder(os.path.join(root, case['folder']), case['ending'])
        assert got == _put(case['result'], root), case


def test_input_and_output_lists_equal_the_references(golden_dir, tmp_path):
    from fast_nnunet_amd import nnUNetPredictor
    doc, root = _golden(golden_dir), str(tmp_path)
    _make_folders(doc, root)
    assert len(doc['manage']) >= 17
    for case in doc['manage']:
        out_dir = os.path.join(root, case['out_dir'])
        os.makedirs(out_dir)
        for f in case['out_files']:
            open(os.path.join(out_dir, f), 'w').close()
        stand_in = types.SimpleNamespace(dataset_json={'file_ending': case['ending']})
        got = nnUNetPredictor._manage_input_and_output_lists(
            stand_in, _put(case['source_arg'], root), _put(case['output_arg'], root),
            os.path.join(root, 'prev') if case['prev'] else None, case['overwrite'], case['part_id'], case['num_parts'],
            case['save_probabilities'])
        assert [list(g) if g is not None else None for g in got] == _put(case['result'], root), case


# ---------------------------------------------------------------------------------------------- ABI
def test_decode_voxels_is_exported_and_the_abi_version_stays_4():
    from fast_nnunet_amd import capi
    assert 'fnn_decode_voxels' in capi.EXPORTS
    lib = capi.load_library()
    assert lib.fnn_abi_version() == 4 and hasattr(lib, 'fnn_decode_voxels')
    # host pointers, a misaligned one and an unknown datatype are refused before anything is launched
    buf = np.zeros(64, np.uint8)
    out = np.zeros(16, np.float32)
    with pytest.raises(AssertionError):
        capi.decode_voxels(buf.ctypes.data + 1, 2, False, 4, False, 1.0, 0.0, out.ctypes.data)
    with pytest.raises(NotImplementedError):
        capi.decode_voxels(buf.ctypes.data - buf.ctypes.data % 16 + 16, 1024, False, 4, False, 1.0, 0.0, out.ctypes.data)
