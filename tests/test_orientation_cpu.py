"""The orientation logic of ``NiftiReorientIO`` without a GPU: orientations, reoriented and restored affines, spacings and
the numpy route through files, against tests/orient_ref.py - whose expected orientations come from how the affines are
constructed, not from the code under test - and the selection of the class by name."""
import os
import warnings

import numpy as np
import pytest

import nifti_ref
import orient_ref as ref

CT = 'example_ct_sm.nii.gz'
SEG = 'example_ct_sm_T300_output.nii.gz'
CASES = [(p, s, rot) for p, s in ref.SIGNED_PERMUTATIONS for rot in (False, True)]
IDS = [f'{"".join(map(str, p))}{"".join("+" if i > 0 else "-" for i in s)}{"_rot" if rot else ""}' for p, s, rot in CASES]


def _affine(perm, signs, rot):
    return ref.affine_of(perm, signs, rot=ref.rotation() if rot else None)


def test_the_yardstick_agrees_with_itself():
    rng = np.random.default_rng(0)
    a = rng.integers(0, 1000, ref.EXTENTS)
    for perm, signs in ref.SIGNED_PERMUTATIONS:
        ornt = ref.ornt_of(perm, signs)
        moved = ref.apply_xyz(a, ornt)
        assert moved.shape == ref.reoriented_shape(ornt, a.shape)
        for idx in ((0, 0, 0), (4, 6, 8), (1, 5, 2)):
            assert moved[ref.map_index(ornt, a.shape, idx)] == a[idx]
        assert np.array_equal(ref.apply_xyz(moved, ref.invert(ornt)), a)
        src, flip = ref.src_axis_flip(ornt)
        zyx = a.transpose(2, 1, 0)
        assert np.array_equal(ref.numpy_reorient(zyx, src, flip), ref.apply_zyx(zyx, ornt))
    assert abs(np.degrees(np.arccos((np.trace(ref.rotation()) - 1) / 2))) < 20          # well inside 45 degrees


@pytest.mark.parametrize('perm, signs, rot', CASES, ids=IDS)
def test_orientation_and_geometry(perm, signs, rot):
    from fast_nnunet_amd import imageio
    affine = _affine(perm, signs, rot)
    shape = ref.EXTENTS
    ornt = imageio.io_orientation(affine)
    assert np.array_equal(ornt, ref.ornt_of(perm, signs)), 'the orientation is the constructed one'
    o = imageio.Reorientation(affine, shape)
    want_aff = ref.reoriented_affine(affine, ornt, shape)
    assert np.allclose(o.reoriented_affine, want_aff, rtol=0, atol=1e-9)
    assert o.ras_shape == ref.reoriented_shape(ornt, shape)[::-1]
    rng = np.random.default_rng(1)
    corners = [(x, y, z) for x in (0, shape[0] - 1) for y in (0, shape[1] - 1) for z in (0, shape[2] - 1)]
    voxels = corners + [tuple(int(rng.integers(0, s)) for s in shape) for _ in range(8)]
    for idx in voxels:
        world = affine @ np.array([*idx, 1.0])
        mapped = ref.map_index(ornt, shape, idx)
        assert np.abs(o.reoriented_affine @ np.array([*mapped, 1.0]) - world).max() <= 1e-9
    rzs = o.reoriented_affine[:3, :3]
    assert np.array_equal(np.argmax(np.abs(rzs), axis=0), [0, 1, 2]) and (np.diag(rzs) > 0).all(), 'positive dominant diagonal'
    assert (o.src_axis, o.flip) == ref.src_axis_flip(ornt)
    assert o.identity == (tuple(perm) == (0, 1, 2) and tuple(signs) == (1, 1, 1))


@pytest.mark.parametrize('perm, signs, rot', CASES, ids=IDS)
def test_round_trip_and_restored_affine(perm, signs, rot):
    from fast_nnunet_amd import imageio
    affine = _affine(perm, signs, rot)
    shape = ref.EXTENTS
    a = np.random.default_rng(2).integers(0, 250, shape[::-1]).astype(np.uint8)            # (z, y, x) of the file
    o = imageio.Reorientation(affine, shape)
    ras = imageio.reorient_on_host(a, o.src_axis, o.flip)
    assert np.array_equal(ras, ref.apply_zyx(a, ref.ornt_of(perm, signs))) and ras.shape == o.ras_shape
    props = {'nibabel_stuff': {'original_affine': o.original_affine, 'reoriented_affine': o.reoriented_affine}}
    src, flip, restored = imageio.restore_orientation(props, ras.shape)
    assert np.array_equal(imageio.reorient_on_host(ras, src, flip), a), 'apply and the way back are the identity'
    assert (src, flip) == ref.src_axis_flip(ref.invert(ref.ornt_of(perm, signs)))
    assert np.allclose(restored, affine)
    assert np.array_equal(restored.astype(np.float32), affine.astype(np.float32)), 'equal after rounding to float32'
    # spacing: the column norms of the reoriented affine in float32, reversed (an identity file: see the file tests)
    norms = np.sqrt((ref.reoriented_affine(affine, ref.ornt_of(perm, signs), shape)[:3, :3] ** 2).sum(0))
    if not o.identity:
        assert o.spacing == [float(np.float32(n)) for n in norms[::-1]]
        zooms = [ref.ZOOMS[list(perm).index(ax)] for ax in range(3)]
        assert np.allclose(o.spacing, zooms[::-1], rtol=1e-6)


def test_ornt_transform_and_inv_ornt_aff_as_published():
    from fast_nnunet_amd import imageio
    for perm, signs in ref.SIGNED_PERMUTATIONS:
        ornt = ref.ornt_of(perm, signs)
        assert np.array_equal(imageio.ornt_transform(imageio.RAS_ORNT, ornt), ref.invert(ornt))
        assert np.array_equal(imageio.ornt_transform(ornt, imageio.RAS_ORNT), ornt)
        assert np.allclose(imageio.inv_ornt_aff(ornt, ref.EXTENTS), ref.index_map(ornt, ref.EXTENTS), atol=1e-12)
        a = np.random.default_rng(3).integers(0, 99, ref.EXTENTS)
        assert np.array_equal(imageio.apply_orientation(a, ornt), ref.apply_xyz(a, ornt))
    assert np.array_equal(imageio.RAS_ORNT, [[0, 1], [1, 1], [2, 1]])
    with pytest.raises(RuntimeError, match='orientation'):
        imageio.io_orientation(np.diag([1.0, 1.0, 0.0, 1.0]))


# ---------------------------------------------------------------------------------------------------------------
# files through the numpy route
# ---------------------------------------------------------------------------------------------------------------
FILE_ORIENTATIONS = [((0, 1, 2), (1, 1, 1)), ((0, 1, 2), (-1, -1, 1)), ((1, 0, 2), (1, -1, -1)), ((2, 1, 0), (-1, 1, 1)),
                     ((1, 2, 0), (1, 1, -1)), ((2, 0, 1), (-1, -1, -1)), ((0, 2, 1), (1, -1, 1))]


def _pixdim(zooms):
    return (1, *zooms)


@pytest.mark.parametrize('perm, signs', FILE_ORIENTATIONS)
@pytest.mark.parametrize('form', ('sform', 'sform_rot', 'qform'))
def test_files_through_the_numpy_route(tmp_path, perm, signs, form):
    from fast_nnunet_amd.imageio import NiftiReorientIO, NiftiIO
    shape_xyz = (6, 7, 9)
    rng = np.random.default_rng(5)
    img = (rng.standard_normal(shape_xyz[::-1]) * 300).astype(np.int16)
    seg = rng.integers(0, 4, shape_xyz[::-1]).astype(np.uint8)
    affine = ref.affine_of(perm, signs, rot=ref.rotation() if form == 'sform_rot' else None)
    f_img, f_seg = str(tmp_path / 'c_0000.nii.gz'), str(tmp_path / 'c.nii.gz')
    if form == 'qform':
        from fast_nnunet_amd.imageio import _quaternion_of
        qfac, zooms, quat = _quaternion_of(affine)
        kw = dict(qform_code=1, quatern=quat, qoffset=tuple(affine[:3, 3]), pixdim=(qfac, *zooms))
    else:
        kw = dict(sform=affine, sform_code=2, pixdim=_pixdim(ref.ZOOMS))
    nifti_ref.write(f_img, img, 4, **kw)
    nifti_ref.write(f_seg, seg, 2, **kw)
    values, info = nifti_ref.read(f_img)
    ornt = ref.closest_axes(info['affine'])
    assert np.array_equal(ornt, ref.ornt_of(perm, signs))
    rw = NiftiReorientIO()
    got, props = rw.read_images([f_img], on_device=False)
    assert got.dtype == np.float32 and np.array_equal(got[0], ref.apply_zyx(values, ornt))
    assert sorted(props) == ['nibabel_stuff', 'spacing'] and sorted(props['nibabel_stuff']) == ['original_affine', 'reoriented_affine']
    assert np.array_equal(props['nibabel_stuff']['original_affine'], info['affine'])
    assert np.allclose(props['nibabel_stuff']['reoriented_affine'], ref.reoriented_affine(info['affine'], ornt, shape_xyz), atol=1e-9)
    if tuple(perm) == (0, 1, 2) and tuple(signs) == (1, 1, 1):
        assert props['spacing'] == info['spacing'] == NiftiIO().read_images([f_img], on_device=False)[1]['spacing']
    else:
        norms = np.sqrt((props['nibabel_stuff']['reoriented_affine'][:3, :3] ** 2).sum(0))
        assert props['spacing'] == [float(np.float32(n)) for n in norms[::-1]]
    ras_seg, seg_props = rw.read_seg(f_seg, on_device=False)
    assert np.array_equal(ras_seg[0], ref.apply_zyx(seg, ornt))
    # the way back: the original voxel bytes, dims and float32 sform
    out = str(tmp_path / 'back.nii.gz')
    with warnings.catch_warnings():
        warnings.simplefilter('error')                       # the restored affine matches: no warning
        rw.write_seg(ras_seg[0].astype(np.uint8), out, seg_props)
    back, back_info = nifti_ref.read(out)
    assert back.dtype == np.uint8 or back.dtype == np.float32
    assert nifti_ref.file_bytes(out)[352:] == seg.tobytes()
    assert tuple(back_info['header']['dim'][1:4]) == shape_xyz
    assert np.array_equal(back_info['sform'].astype(np.float32), info['affine'].astype(np.float32))
    assert int(back_info['header']['sform_code']) == 2 and int(back_info['header']['qform_code']) == 0


def test_a_case_of_files_that_disagree_after_reorientation(tmp_path):
    from fast_nnunet_amd.imageio import NiftiReorientIO
    a = np.zeros((5, 6, 7), np.int16)
    f0, f1, f2 = (str(tmp_path / f'd_000{i}.nii') for i in range(3))
    nifti_ref.write(f0, a, 4, sform=ref.affine_of((0, 1, 2), (1, 1, 1)), sform_code=1, pixdim=_pixdim(ref.ZOOMS))
    # the same voxels stored x <-> y swapped: another file shape, the same reoriented shape and spacing
    nifti_ref.write(f1, a.transpose(0, 2, 1), 4, sform=ref.affine_of((1, 0, 2), (1, 1, 1), zooms=(1.3, 0.7, 2.5)), sform_code=1,
                    pixdim=(1, 1.3, 0.7, 2.5))
    got, _ = NiftiReorientIO().read_images([f0, f1], on_device=False)
    assert got.shape == (2, 5, 6, 7)
    nifti_ref.write(f2, a, 4, sform=ref.affine_of((1, 0, 2), (1, 1, 1)), sform_code=1, pixdim=_pixdim(ref.ZOOMS))
    with pytest.raises(RuntimeError, match='same shape'):
        NiftiReorientIO().read_images([f0, f2], on_device=False)
    nifti_ref.write(f2, a, 4, sform=ref.affine_of((0, 1, 2), (-1, 1, 1), zooms=(0.8, 1.3, 2.5)), sform_code=1, pixdim=(1, 0.8, 1.3, 2.5))
    with pytest.raises(RuntimeError, match='spacing'):
        NiftiReorientIO().read_images([f0, f2], on_device=False)
    nifti_ref.write(f2, a, 4, sform=ref.affine_of((0, 1, 2), (1, 1, 1), origin=(0, 0, 0)), sform_code=1, pixdim=_pixdim(ref.ZOOMS))
    with pytest.warns(UserWarning, match='reoriented_affines'):
        NiftiReorientIO().read_images([f0, f2], on_device=False)


def test_write_seg_warns_when_the_restored_affine_is_not_the_original(tmp_path):
    from fast_nnunet_amd.imageio import NiftiReorientIO
    affine = ref.affine_of((1, 0, 2), (1, -1, 1))
    other = affine.copy()
    other[0, 3] += 5.0
    from fast_nnunet_amd.imageio import Reorientation
    o = Reorientation(other, (4, 5, 6))
    props = {'nibabel_stuff': {'original_affine': affine, 'reoriented_affine': o.reoriented_affine}}
    with pytest.warns(UserWarning, match='Restored affine'):
        NiftiReorientIO().write_seg(np.zeros(o.ras_shape, np.uint8), str(tmp_path / 'w.nii.gz'), props)
    assert nifti_ref.read(str(tmp_path / 'w.nii.gz'))[1]['shape'] == (6, 5, 4)


def test_the_ct_fixture_is_ras_already(golden_dir, tmp_path):
    from fast_nnunet_amd.imageio import NiftiReorientIO, NiftiIO, Reorientation, read_header
    f = os.path.join(golden_dir, CT)
    hdr = read_header(f)
    assert np.array_equal(hdr.affine[:3, :3], np.diag([3.0, 3.0, 3.0])) and Reorientation(hdr.affine, hdr.shape_xyz).identity
    got, props = NiftiReorientIO().read_images([f], on_device=False)
    want, want_props = NiftiIO().read_images([f], on_device=False)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)) and props['spacing'] == want_props['spacing']
    assert np.array_equal(props['nibabel_stuff']['original_affine'], want_props['nibabel_stuff']['original_affine'])
    assert np.array_equal(props['nibabel_stuff']['reoriented_affine'], props['nibabel_stuff']['original_affine'])
    labels = nifti_ref.read(os.path.join(golden_dir, SEG))[0].astype(np.uint8)
    out = str(tmp_path / 'labels.nii.gz')
    NiftiReorientIO().write_seg(labels, out, props)
    assert open(out, 'rb').read() == open(os.path.join(golden_dir, SEG), 'rb').read(), 'byte for byte the reference\'s file'


# ---------------------------------------------------------------------------------------------------------------
# selection
# ---------------------------------------------------------------------------------------------------------------
def _plans_manager(name=None):
    from fast_nnunet_amd.plans import PlansManager
    plans = {'dataset_name': 'Dataset997_Orient', 'plans_name': 'nnUNetPlans', 'transpose_forward': [0, 1, 2],
             'transpose_backward': [0, 1, 2], 'foreground_intensity_properties_per_channel': {}, 'configurations': {}}
    if name is not None:
        plans['image_reader_writer'] = name
    return PlansManager(plans)


def test_selection():
    from fast_nnunet_amd import imageio
    from fast_nnunet_amd.imageio import prediction_reader_writer_class as resolve
    dj = {'file_ending': '.nii.gz'}
    assert resolve(_plans_manager('NibabelIOWithReorient'), dj) is imageio.NiftiReorientIO
    assert resolve(_plans_manager(), dict(dj, overwrite_image_reader_writer='NibabelIOWithReorient')) is imageio.NiftiReorientIO
    assert resolve(_plans_manager('NibabelIO'), dict(dj, overwrite_image_reader_writer='NibabelIOWithReorient')) is imageio.NiftiReorientIO
    assert resolve(_plans_manager('NibabelIO'), dj) is imageio.NiftiIO and resolve(_plans_manager('SimpleITKIO'), dj) is imageio.NiftiIO
    assert resolve(_plans_manager(), dj) is imageio.NiftiIO
    assert resolve(_plans_manager(), dict(dj, overwrite_image_reader_writer='SimpleITKIO')) is imageio.NiftiIO
    assert issubclass(imageio.NiftiReorientIO, imageio.NiftiIO)
    # the registry mirrors keep refusing the name
    with pytest.raises(NotImplementedError, match='NibabelIOWithReorient'):
        imageio.reader_writer_class_by_name('NibabelIOWithReorient')
    with pytest.raises(NotImplementedError, match='NibabelIOWithReorient'):
        imageio.determine_reader_writer_from_dataset_json(dict(dj, overwrite_image_reader_writer='NibabelIOWithReorient'))
    with pytest.raises(NotImplementedError, match='NibabelIOWithReorient'):
        _plans_manager('NibabelIOWithReorient').image_reader_writer_class
    # the ITK one stays out, whoever is asked
    with pytest.raises(NotImplementedError, match='SimpleITKIOWithReorient'):
        imageio.reader_writer_class_by_name('SimpleITKIOWithReorient')
    with pytest.raises(NotImplementedError, match='SimpleITKIOWithReorient'):
        resolve(_plans_manager('SimpleITKIOWithReorient'), dj)
    with pytest.raises(NotImplementedError, match='SimpleITKIOWithReorient'):
        resolve(_plans_manager(), dict(dj, overwrite_image_reader_writer='SimpleITKIOWithReorient'))
    with pytest.raises(NotImplementedError):
        resolve(_plans_manager('Tiff3DIO'), dj)


def test_reorient_is_exported_and_the_abi_version_stays_4():
    from fast_nnunet_amd import capi
    assert 'fnn_reorient' in capi.EXPORTS
    lib = capi.load_library()
    assert lib.fnn_abi_version() == 4 and hasattr(lib, 'fnn_reorient')
    # refused before any launch, without a GPU: a host pointer, and what the arguments alone show
    a, out = np.zeros(64, np.uint8), np.zeros(64, np.uint8)
    with pytest.raises(AssertionError, match='device'):
        capi.reorient(a.ctypes.data, 1, (2, 3, 4), (2, 0, 1), (0, 1, 0), out.ctypes.data)
    with pytest.raises(NotImplementedError, match='1, 2 or 4'):
        capi.reorient(a.ctypes.data, 8, (2, 3, 4), (2, 0, 1), (0, 1, 0), out.ctypes.data)
    with pytest.raises(AssertionError, match='permutation'):
        capi.reorient(a.ctypes.data, 1, (2, 3, 4), (2, 0, 0), (0, 1, 0), out.ctypes.data)
    with pytest.raises(AssertionError, match='overlap'):
        capi.reorient(a.ctypes.data, 1, (2, 3, 4), (2, 0, 1), (0, 1, 0), a.ctypes.data + 8)
    capi.reorient(a.ctypes.data, 1, (2, 0, 4), (2, 0, 1), (0, 1, 0), out.ctypes.data)       # no elements: nothing to do
    assert not out.any()
