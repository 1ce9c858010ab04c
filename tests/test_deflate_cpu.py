"""The device deflate route without a GPU: the C ABI, the host assembly of the ``.nii.gz`` member around a fragment, the
CRC-32 combine, the capacity bound and the size condition - on fragments made by the Python model of the encoder
(tests/deflate_ref.py), which the GPU tests compare with the kernels byte for byte."""
import gzip
import os
import re
import zlib

import numpy as np
import pytest

import deflate_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MASK = 'example_ct_sm_T300_output.nii.gz'
AFFINE = np.array([[0.0, -2.5, 0.0, 11.0], [3.0, 0.0, 0.0, -20.5], [0.0, 0.0, 1.5, 7.0], [0.0, 0.0, 0.0, 1.0]])


def test_the_library_exports_the_deflate_entry_points_in_abi_4():
    from fast_nnunet_amd import capi
    header = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'fnn.h')).read(), flags=re.S)
    lib = capi.load_library()
    for name in ('fnn_deflate_bound', 'fnn_deflate_labels'):
        assert re.search(r'\b' + name + r'\s*\(', header) and name in capi.EXPORTS and hasattr(lib, name)
    assert lib.fnn_abi_version() == 4


def test_bound_is_the_models_and_holds_on_nine_bit_literals():
    """Bytes from 144 on take 9-bit literals; without a run among them nothing is shorter than that."""
    from fast_nnunet_amd import capi
    S, C = deflate_ref.SEGMENT, deflate_ref.CHUNK
    rng = np.random.default_rng(3)
    for n in (0, 1, 2, 7, 8, S, C - 1, C, C + 1, 3 * C + 5):
        assert capi.deflate_bound(n) == deflate_ref.bound(n)
        data = rng.integers(144, 256, n, dtype=np.uint8).tobytes()
        for elem in (1, 2) if n % 2 == 0 else (1,):
            frag = deflate_ref.fragment(data, elem)
            assert len(frag) <= capi.deflate_bound(n), (n, elem)
            assert deflate_ref.inflate(frag) == data
    worst = bytes(range(144, 256)) * (2 * C // 112 + 1)                     # no byte equals its neighbour: literals only
    for n in (C, 2 * C):
        assert len(deflate_ref.fragment(worst[:n], 1)) == capi.deflate_bound(n), 'the bound is reached'
    assert capi.deflate_bound(-5) == 0 and capi.deflate_bound(2 ** 40) == 9 * 2 ** 37 + 6 * 2 ** 26


@pytest.mark.parametrize('n', (0, 1, 255, 256, 65537))
def test_crc_combine_is_the_crc_of_the_concatenation(n):
    from fast_nnunet_amd import imageio
    rng = np.random.default_rng(n)
    for la in (0, 1, 352, 4097):
        a, b = rng.bytes(la), rng.bytes(n)
        want = zlib.crc32(a + b)
        assert imageio.crc32_combine(zlib.crc32(a), zlib.crc32(b), n) == want
        assert deflate_ref.crc_combine(zlib.crc32(a), zlib.crc32(b), n) == want


def _model_labels(voxels, affine):
    """What ``NiftiIO.compress_labels`` returns, with the model in the kernel's place."""
    from fast_nnunet_amd.imageio import DeviceCompressedLabels, _label_voxels
    data, u16 = _label_voxels(voxels)
    raw = data.tobytes()
    return DeviceCompressedLabels(deflate_ref.fragment(raw, 2 if u16 else 1), zlib.crc32(raw), len(raw), data.shape, u16, affine)


def _label_maps():
    rng = np.random.default_rng(9)
    blocks = np.repeat(np.repeat(rng.integers(0, 5, (5, 6, 7)), 4, 1), 9, 2)            # (5, 24, 63): runs along x
    return {'uint8': blocks.astype(np.uint8),
            'uint16': (blocks * 300).astype(np.uint16),                                  # maximum >= 255: a uint16 file
            'narrowed': (blocks * 60).astype(np.uint16)}                                 # maximum 240: written as uint8


@pytest.mark.parametrize('kind', ('uint8', 'uint16', 'narrowed'))
def test_assembled_file_inflates_to_todays_file(tmp_path, kind):
    from fast_nnunet_amd import imageio
    seg = _label_maps()[kind]
    today, device = str(tmp_path / 'today.nii.gz'), str(tmp_path / 'device.nii.gz')
    imageio.write_label_file(seg, today, AFFINE)
    labels = _model_labels(seg, AFFINE)
    assert labels.uint16 == (kind == 'uint16') and labels.n_bytes == seg.size * (2 if kind == 'uint16' else 1)
    imageio.write_label_file(labels, device, AFFINE)
    a, b = open(today, 'rb').read(), open(device, 'rb').read()
    assert a[:10] == b[:10] == imageio.GZIP_HEADER and a != b
    plain = gzip.decompress(b)
    assert plain == gzip.decompress(a), 'the same 352-byte header and the same voxels'
    assert plain[:352] == imageio.nifti1_header_bytes(seg.shape[::-1], 512 if kind == 'uint16' else 2, AFFINE)
    assert plain[352:] == seg.astype('<u2' if kind == 'uint16' else np.uint8).tobytes()
    # one member, nothing behind it; the reader of this package reads it
    d = zlib.decompressobj(31)
    assert d.decompress(b) == plain and d.eof and d.unused_data == b''
    got, props = imageio.NiftiIO().read_seg(device, on_device=False)
    assert np.array_equal(got[0], seg) and np.allclose(props['nibabel_stuff']['original_affine'], AFFINE)
    # write_seg of both reader-writers takes the value; the header's affine is the one it carries
    imageio.NiftiIO().write_seg(labels, str(tmp_path / 'w.nii.gz'), {})
    imageio.NiftiReorientIO().write_seg(labels, str(tmp_path / 'r.nii.gz'), {})
    assert open(tmp_path / 'w.nii.gz', 'rb').read() == open(tmp_path / 'r.nii.gz', 'rb').read() == b
    assert not [f for f in os.listdir(tmp_path) if '.part' in f]


def test_compressed_labels_make_no_plain_nii_and_leave_nothing_behind(tmp_path):
    from fast_nnunet_amd import imageio
    labels = _model_labels(_label_maps()['uint8'], AFFINE)
    with pytest.raises(ValueError, match='.nii.gz'):
        imageio.write_label_file(labels, str(tmp_path / 'x.nii'), AFFINE)
    assert os.listdir(tmp_path) == []
    with pytest.raises(TypeError, match='GPU'):
        imageio.NiftiIO().compress_labels(_label_maps()['uint8'], {})                  # a numpy array takes today's route


def test_size_condition_on_the_golden_mask(golden_dir):
    """The fragment is at most twice zlib level 1: the cap that guards against slicing too finely."""
    voxels = gzip.decompress(open(os.path.join(golden_dir, MASK), 'rb').read())[352:]
    for elem, raw in ((1, voxels), (2, np.frombuffer(voxels, np.uint8).astype('<u2').tobytes())):
        frag = deflate_ref.fragment(raw, elem)
        ratio = len(frag) / len(zlib.compress(raw, 1))
        print(f'golden mask as {elem}-byte labels: {len(frag)} B, {ratio:.2f} x zlib level 1')
        assert deflate_ref.inflate(frag) == raw and ratio <= 2.0


def test_model_tokens_follow_the_rule():
    t = deflate_ref.tokens
    assert t(b'\x05' * 2, 1) == [('lit', 5), ('lit', 5)]
    assert t(b'\x05' * 3, 1) == [('lit', 5), ('lit', 5), ('lit', 5)], 'two repeats are no match'
    assert t(b'\x05' * 4, 1) == [('lit', 5), ('match', 3)]
    assert t(b'\x05' * 256, 1) == [('lit', 5), ('match', 255)]
    assert t(b'\x01\x02' * 3 + b'\x09', 2) == [('lit', 1), ('lit', 2), ('match', 4), ('lit', 9)]
    assert t(b'\x01\x01\x02\x02\x02\x02\x03', 1) == [('lit', 1), ('lit', 1), ('lit', 2), ('match', 3), ('lit', 3)]
    # a run that crosses a segment edge starts again with a literal; chunks are independent streams
    S, C = deflate_ref.SEGMENT, deflate_ref.CHUNK
    data = b'\x07' * (C + 5)
    assert deflate_ref.fragment(data, 1) == deflate_ref.chunk_bytes(data[:C], 1) + deflate_ref.chunk_bytes(data[C:], 1)
    assert deflate_ref.inflate(deflate_ref.chunk_bytes(data[C:], 1)) == data[C:]
    assert deflate_ref.chunk_bytes(data[:S], 1)[-4:] == b'\x00\x00\xff\xff'
