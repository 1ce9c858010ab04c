"""The per-label mask route without a GPU: the C ABI, the Python model of the mask fragment (tests/deflate_masks_ref.py, which
the GPU tests compare with the kernels byte for byte), the host assembly of a mask file around a model fragment, the size of
the work buffer, and ``JHUPredictor``'s file names and its refusal of region-based datasets."""
import gzip
import os
import re
import zlib

import numpy as np
import pytest

import deflate_masks_ref as masks_ref
import deflate_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MASK = 'example_ct_sm_T300_output.nii.gz'
AFFINE = np.array([[0.0, -2.5, 0.0, 11.0], [3.0, 0.0, 0.0, -20.5], [0.0, 0.0, 1.5, 7.0], [0.0, 0.0, 0.0, 1.0]])
C = deflate_ref.CHUNK
NAMES = ('fnn_deflate_masks_work_bytes', 'fnn_deflate_masks_count', 'fnn_deflate_masks_emit')


def test_the_library_exports_the_mask_entry_points_in_abi_4():
    from fast_nnunet_amd import capi
    header = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'fnn.h')).read(), flags=re.S)
    lib = capi.load_library()
    for name in NAMES:
        assert re.search(r'\b' + name + r'\s*\(', header) and name in capi.EXPORTS and hasattr(lib, name), name
    assert lib.fnn_abi_version() == 4


def test_zero_chunk_is_112_bytes_and_inflates_to_a_chunk_of_zeros():
    z = masks_ref.ZERO_CHUNK
    assert len(z) == masks_ref.ZERO_CHUNK_BYTES == 112
    assert len(deflate_ref.chunk_bytes(bytes(C), 1)) == 214, 'what the segment rule takes for the same chunk'
    assert deflate_ref.inflate(z) == bytes(C)
    assert deflate_ref.inflate(z * 5) == bytes(5 * C), 'a run of zero chunks is a run of zeros'
    assert z[-4:] == b'\x00\x00\xff\xff'
    assert 64 * 112 * 128 == 917504, 'an empty 512^3 mask: 8192 chunks'


def _small_maps():
    rng = np.random.default_rng(19)
    blocks = np.repeat(rng.choice((0, 1, 2, 5), 700), rng.choice((3, 40, 300, 900), 700))[:3 * C + 5]
    sparse = np.zeros(4 * C, np.int64)
    sparse[C] = 3                                                   # the first byte of a chunk ...
    sparse[3 * C - 1] = 4                                           # ... and the last byte of one
    sparse[C + 100:C + 400] = 9
    wide = np.repeat(rng.choice((1, 257, 513), 300), rng.choice((1, 2, 3, 200), 300))[:2 * C + 77]
    return {'blocks_uint8': (blocks.astype(np.uint8), (0, 1, 2, 5, 7, 300)),
            'sparse_uint8': (sparse.astype(np.uint8), (0, 3, 4, 9, 11)),
            'uint16': (wide.astype(np.uint16), (1, 257, 513, 2, 0)),
            'one_partial_chunk': (blocks[:255].astype(np.uint8), (0, 1, 7))}


def _check_fragments(seg, labels, where):
    for label in labels:
        mask = masks_ref.mask_of(seg, label).tobytes()
        frag = masks_ref.mask_fragment(seg, label)
        assert deflate_ref.inflate(frag) == mask, f'{where}, label {label}: the fragment does not inflate to the mask'
        assert len(frag) <= len(deflate_ref.fragment(mask, 1)), f'{where}, label {label}: longer than the segment rule'


@pytest.mark.parametrize('kind', sorted(_small_maps()))
def test_model_fragments_inflate_to_the_masks_and_are_no_longer_than_the_segment_rule(kind):
    seg, labels = _small_maps()[kind]
    _check_fragments(seg, labels, kind)
    absent = [l for l in labels if not (seg == l).any()]
    assert absent, 'a label that occurs nowhere is among them'
    full, tail = divmod(seg.size, C)
    for label in absent:
        frag = masks_ref.mask_fragment(seg, label)
        assert frag[:112 * full] == masks_ref.ZERO_CHUNK * full
        assert frag[112 * full:] == (deflate_ref.chunk_bytes(bytes(tail), 1) if tail else b''), 'the last partial chunk is tokenised'


def test_model_fragments_of_the_golden_mask(golden_dir):
    voxels = np.frombuffer(gzip.decompress(open(os.path.join(golden_dir, MASK), 'rb').read())[352:], np.uint8)
    labels = sorted(set(np.unique(voxels).tolist()) | {0, 200})
    _check_fragments(voxels, labels, 'golden mask')
    per_chunk = [np.unique(voxels[c:c + C]).size for c in range(0, voxels.size, C)]
    print(f'golden mask: {len(per_chunk)} chunks, labels per chunk {min(per_chunk)} .. {max(per_chunk)}; '
          f'{masks_ref.present_pairs(voxels, labels)} of {len(labels) * len(per_chunk)} (chunk, label) pairs are walked')


def test_assembled_mask_file_decompresses_to_the_host_writers_mask_file(tmp_path):
    from fast_nnunet_amd import imageio
    rng = np.random.default_rng(9)
    seg = np.repeat(np.repeat(rng.integers(0, 5, (5, 6, 7)), 4, 1), 9, 2).astype(np.uint8)     # (5, 24, 63): runs along x
    for label in (0, 3, 77):
        mask = (seg == label).astype(np.uint8)
        today, device = str(tmp_path / f'today{label}.nii.gz'), str(tmp_path / f'device{label}.nii.gz')
        imageio.write_label_file(mask, today, AFFINE)
        labels = imageio.DeviceCompressedLabels(masks_ref.mask_fragment(seg, label), zlib.crc32(mask.tobytes()), mask.size,
                                                mask.shape, False, AFFINE)
        blob = imageio.compressed_label_file_bytes(labels)
        assert gzip.decompress(blob) == gzip.decompress(open(today, 'rb').read())
        imageio.NiftiIO().write_seg(labels, device, {})
        assert open(device, 'rb').read() == blob
        got, _ = imageio.NiftiIO().read_seg(device, on_device=False)
        assert got.dtype == np.float32 and np.array_equal(got[0], mask)
    assert not [f for f in os.listdir(tmp_path) if '.part' in f]


def test_work_bytes_is_the_stated_formula():
    from fast_nnunet_amd import capi
    for n in (0, 1, C - 1, C, C + 1, 3 * C + 5, 512 ** 3):
        for n_labels in (1, 3, 33, 118, 65536):
            assert capi.deflate_masks_work_bytes(n, n_labels) == masks_ref.work_bytes(n, n_labels), (n, n_labels)
    assert masks_ref.work_bytes(512 ** 3, 118) == 384 + 480 + 960 + 944 + 480 + 10 * 118 * 8192
    assert capi.deflate_masks_work_bytes(-1, 3) == 0 and capi.deflate_masks_work_bytes(5, 0) == 0
    assert capi.deflate_masks_work_bytes(5, 65537) == 0, 'more labels than values: one is named twice'


def _toy_label_manager(labels):
    from fast_nnunet_amd.plans import PlansManager
    pm = PlansManager({'dataset_name': 'Dataset998_Masks', 'plans_name': 'nnUNetPlans', 'configurations': {'3d_fullres': {
        'patch_size': [16, 16, 32], 'architecture': {'network_class_name': 'PlainConvUNet', 'arch_kwargs': {}, '_kw_requires_import': []}}}})
    dj = {'labels': labels, 'channel_names': {'0': 'CT'}, 'file_ending': '.nii.gz'}
    return pm, dj


def test_mask_file_names_of_a_toy_dataset():
    from fast_nnunet_amd.jhu import JHUPredictor, mask_file_names
    from fast_nnunet_amd import nnUNetPredictor
    pm, dj = _toy_label_manager({'background': 0, 'liver': 1, 'kidney_left': 2, 'aorta': 5})
    lm = pm.get_label_manager(dj)
    names = mask_file_names(lm, dj, os.path.join('out', 'case7'))
    folder = os.path.join('out', 'case7', 'predictions')
    assert names == [(1, os.path.join(folder, 'liver.nii.gz')), (2, os.path.join(folder, 'kidney_left.nii.gz')),
                     (5, os.path.join(folder, 'aorta.nii.gz'))]
    assert mask_file_names(lm, dict(dj, file_ending='.nii'), 'x')[0] == (1, os.path.join('x', 'predictions', 'liver.nii'))
    assert issubclass(JHUPredictor, nnUNetPredictor)


def test_region_based_datasets_are_refused_before_any_gpu_work():
    from fast_nnunet_amd.jhu import JHUPredictor, mask_file_names
    pm, dj = _toy_label_manager({'background': 0, 'whole': [1, 2, 3], 'core': [2, 3], 'enhancing': 3})
    dj['regions_class_order'] = [1, 2, 3]
    lm = pm.get_label_manager(dj)
    assert lm.has_regions
    with pytest.raises(NotImplementedError, match='region'):
        mask_file_names(lm, dj, 'x')
    p = JHUPredictor(device='cuda', allow_tqdm=False)                # (constructing the predictor touches no GPU)
    with pytest.raises(NotImplementedError, match='region'):
        p.manual_initialization(None, pm, pm.get_configuration('3d_fullres'), [{}], dj, 'nnUNetTrainer', None)
    assert p._engine is None, 'refused before the engine was built'
