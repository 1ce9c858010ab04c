"""The device inflate on a real MI355X: ``fnn_inflate_segments`` (csrc/inflate.hip: inflate_count_kernel,
inflate_emit_kernel) against zlib byte for byte and against the Python model of the segment rule and the chain
(tests/inflate_ref.py) status for status - round trips with both device encoders, zlib's Z_FIXED full-flush streams, false
candidates, refusals - and the label-file readers and folder commands with ``inflate_on_device=True`` against the route
they take without it.

Every call runs between guard bands: 64 bytes of a pattern in front of and behind ``in`` and ``out``, which must be
unchanged afterwards.  The malformed streams here are data a decoder has to refuse with a status word; none of them is
meant to, or may, provoke a fault.
"""
import gzip
import json
import os
import zlib

import numpy as np
import pytest
import torch

import deflate_masks_ref as masks_ref
import inflate_ref as ref

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda', 0)
C = ref.SEGMENT_MAX
SIZES = (1, 255, 256, 257, C - 1, C, C + 1, 3 * C + 5)
GUARD, FILL = 64, 0xA5


def _stream():
    return torch.cuda.current_stream(DEV).cuda_stream


def _inflate(stream: bytes, starts, out_bytes: int, in_bytes=None):
    """One call between guard bands -> (status, crc32, the bytes of ``out``)."""
    from fast_nnunet_amd import capi
    in_bytes = len(stream) if in_bytes is None else in_bytes
    src = torch.full((GUARD + len(stream) + GUARD,), FILL, dtype=torch.uint8, device=DEV)
    if stream:
        src[GUARD:GUARD + len(stream)] = torch.frombuffer(bytearray(stream), dtype=torch.uint8).to(DEV)
    dst = torch.full((GUARD + out_bytes + GUARD,), FILL, dtype=torch.uint8, device=DEV)
    assert (src.data_ptr() + GUARD) % 16 == 0 and (dst.data_ptr() + GUARD) % 16 == 0
    before = src.cpu().numpy().copy()
    status, crc = capi.inflate_segments(src.data_ptr() + GUARD, in_bytes, starts, dst.data_ptr() + GUARD, out_bytes, _stream())
    host = dst.cpu().numpy()
    assert np.all(host[:GUARD] == FILL) and np.all(host[GUARD + out_bytes:] == FILL), 'wrote outside out[0, out_bytes)'
    assert np.array_equal(src.cpu().numpy(), before), 'the input and its guard bands are left alone'
    return status, crc, host[GUARD:GUARD + out_bytes].tobytes()


def _served(stream: bytes, starts, data: bytes):
    from fast_nnunet_amd import capi
    status, crc, out = _inflate(stream, starts, len(data))
    assert status == 0, ref.REASONS[status]
    assert out == data
    assert crc == zlib.crc32(data)
    if stream:
        assert capi.op_last_kernels() == ['inflate_count_kernel', 'inflate_emit_kernel']


def _refused(stream: bytes, starts, out_bytes: int, reason: int, in_bytes=None):
    from fast_nnunet_amd import capi
    assert ref.chain(stream[:in_bytes], starts, out_bytes)[0] == reason, 'the model'
    status, crc, _ = _inflate(stream, starts, out_bytes, in_bytes)
    assert (ref.REASONS[status], crc) == (ref.REASONS[reason], 0)
    assert capi.op_last_kernels() == ['inflate_count_kernel'], 'nothing is launched past the point of knowing'


DATA = {
    'zeros': lambda n, elem: bytes(n * elem),
    'runs': lambda n, elem: ref.label_runs(n * elem, elem, seed=n),
    'random': lambda n, elem: ref.random_bytes(n * elem, seed=n),                       # literals of 9 bits among them
    'above_255': lambda n, elem: (np.repeat(np.arange(n // 7 + 1) % 5 * 300 + 256, 7)[:n]).astype('<u2').tobytes(),
}


def _device_fragment(data: bytes, elem: int):
    from fast_nnunet_amd import capi
    n = len(data) // elem
    src = torch.frombuffer(bytearray(data), dtype=torch.uint8).to(DEV)
    cap = capi.deflate_bound(len(data))
    buf = torch.empty(cap, dtype=torch.uint8, device=DEV)
    n_out, file_size, crc = capi.deflate_labels(src.data_ptr(), elem, n, False, buf.data_ptr(), cap, _stream())
    assert file_size == elem
    return buf[:n_out].cpu().numpy().tobytes(), crc


@pytest.mark.parametrize('kind,elem', [('zeros', 1), ('runs', 1), ('random', 1), ('zeros', 2), ('runs', 2), ('random', 2), ('above_255', 2)])
def test_round_trip_with_the_label_encoder(kind, elem):
    for n in SIZES + ((C // 2, C // 2 + 1) if elem == 2 else ()):
        data = DATA[kind](n, elem)
        frag, crc = _device_fragment(data, elem)
        assert crc == zlib.crc32(data)
        _served(frag, ref.candidates(frag), data)


@pytest.mark.parametrize('dtype', ['u1', '<u2'])
def test_round_trip_with_the_mask_encoder(dtype):
    """Label 2 occurs in every chunk, 6 (2-byte map: 300) in one - the full chunks around it are the constant zero chunk,
    matches of 258 at distance 1 - and 9 nowhere."""
    from fast_nnunet_amd import capi
    m = (np.arange(3 * C + 5) // 37 % 5).astype(dtype)
    one = 6 if m.itemsize == 1 else 300
    m[C + 700:C + 900] = one
    labels = [2, one, 9]
    src = torch.frombuffer(bytearray(m.tobytes()), dtype=torch.uint8).to(DEV)
    work_cap = capi.deflate_masks_work_bytes(m.size, len(labels))
    work = torch.empty(work_cap, dtype=torch.uint8, device=DEV)
    sizes, crcs = capi.deflate_masks_count(src.data_ptr(), m.itemsize, m.size, labels, work.data_ptr(), work_cap, _stream())
    out = torch.empty(sum(sizes), dtype=torch.uint8, device=DEV)
    capi.deflate_masks_emit(src.data_ptr(), m.itemsize, m.size, labels, work.data_ptr(), out.data_ptr(), sum(sizes), _stream())
    blob, at = out.cpu().numpy().tobytes(), 0
    for label, nb, crc in zip(labels, sizes, crcs):
        frag, at = blob[at:at + nb], at + nb
        mask = masks_ref.mask_of(m, label).tobytes()
        assert crc == zlib.crc32(mask)
        if label != 2:
            assert frag.startswith(masks_ref.ZERO_CHUNK)
        _served(frag, ref.candidates(frag), mask)


ZLIB_DATA = {'texty': lambda: ref.texty_bytes(40000, 1), 'random': lambda: ref.random_bytes(20000, 2), 'runs': lambda: ref.label_runs(40000, 2, 5)}


@pytest.mark.parametrize('name', sorted(ZLIB_DATA))
@pytest.mark.parametrize('level', [1, 9])
def test_zlib_fixed_full_flush_streams(name, level):
    """Matches of general distance and length, overlapping ones (the 2-byte runs: distance 2, lengths to 258) and, on random
    bytes, stored blocks with data.  k = 100 puts most segments at offsets of ``out`` that are no multiple of 16."""
    for k in (100, 4096, 16384):
        data = ZLIB_DATA[name]()[:3000 if k == 100 else None]
        stream = ref.full_flush_stream(data, level, k)
        assert ref.inflate_raw(stream) == data
        if name == 'random':
            assert stream[0] & 7 == 0, 'a stored block'
        _served(stream, ref.candidates(stream), data)


def test_empty_inputs_launch_nothing():
    from fast_nnunet_amd import capi
    assert _inflate(b'', [], 0)[:2] == (0, 0)
    assert capi.op_last_kernels() == []
    assert _inflate(b'', [], 5)[:2] == (ref.SIZE, 0)
    assert _inflate(b'\x00\x00\x00\xff\xff', [], 0)[:2] == (0, 0)
    assert capi.op_last_kernels() == []
    _served(b'\x00\x00\x00\xff\xff', [0], b'')                    # one segment that makes nothing


@pytest.mark.parametrize('name', ['labels', 'zlib-texty', 'zlib-random'])
def test_every_byte_position_as_a_candidate(name):
    """A stream of at most 4 KiB in which every byte is a candidate: the false ones decode to whatever they decode to and
    are ignored.  Segments behind the first land at offsets of ``out`` that are no multiple of 16."""
    if name == 'labels':
        data = ref.label_runs(3 * C + 5, 1, seed=11)
        stream, _ = _device_fragment(data, 1)
    else:
        data = (ref.texty_bytes(3000, 1) if name == 'zlib-texty' else ref.random_bytes(3000, 2))
        stream = ref.full_flush_stream(data, 9, 100)
    assert len(stream) <= 4096
    if name != 'labels':                                           # (the encoders' chunks all begin at multiples of 16 KiB)
        ends = [ref.decode_segment(stream, s)[0] for s in ref.candidates(stream)]
        assert any(len(ref.inflate_raw(stream[:e])) % 16 for e in ends[:-1]), 'a member at an offset that is no multiple of 16'
    _served(stream, list(range(len(stream))), data)


def test_refusals_are_a_status_word():
    texty = ref.texty_bytes(40000, 1)
    s = ref.full_flush_stream(texty, 6, 4096, zlib.Z_DEFAULT_STRATEGY)
    _refused(s, ref.candidates(s), len(texty), ref.DYNAMIC)
    s = ref.full_flush_stream(texty, 6, 4096, flush=zlib.Z_SYNC_FLUSH)                  # (Z_FIXED: distances cross the segments)
    _refused(s, ref.candidates(s), len(texty), ref.DISTANCE)
    s = ref.full_flush_stream(texty, 1, C + 1)
    _refused(s, ref.candidates(s), len(texty), ref.OUTPUT)
    a = ref.full_flush_stream(texty[:1000], 1, 1000)
    z = zlib.compressobj(1, zlib.DEFLATED, -15, 8, zlib.Z_FIXED)
    s = a + z.compress(texty[1000:2000]) + z.flush() + a                               # a finished stream in the middle
    _refused(s, ref.candidates(s), 3000, ref.FINAL)
    s = ref.full_flush_stream(texty, 1, 4096)
    _refused(s + b'\x01\x02\x03', ref.candidates(s), len(texty), ref.CHAIN)              # the chain ends 3 bytes short of in_bytes
    _refused(s, ref.candidates(s), len(texty), ref.END, in_bytes=len(s) - 3)            # the input ends inside the last segment
    _refused(s, ref.candidates(s), len(texty) + 1, ref.SIZE)
    _refused(s, ref.candidates(s), len(texty) - 1, ref.SIZE)
    _served(s, ref.candidates(s), texty)


def test_two_calls_give_identical_bytes():
    data = ref.label_runs(3 * C + 6, 2, seed=3)
    stream, _ = _device_fragment(data, 2)
    first = _inflate(stream, ref.candidates(stream), len(data))
    assert first == _inflate(stream, ref.candidates(stream), len(data)) and first[2] == data


# ---------------------------------------------------------------------------------------------------------------
# files: label and mask files written on the device, read back with the flag off and on
# ---------------------------------------------------------------------------------------------------------------
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
SHAPE = (20, 33, 47)
RAS = np.diag([1.5, 2.0, 0.5, 1.0])
NOT_RAS = np.array([[0.0, -2.0, 0.0, 5.0], [1.5, 0.0, 0.0, -3.0], [0.0, 0.0, -0.5, 7.0], [0.0, 0.0, 0.0, 1.0]])
PLANS = {'dataset_name': 'd', 'plans_name': 'p', 'image_reader_writer': 'NibabelIO', 'configurations': {}}
DATASET = {'labels': {'background': 0, 'a': 1, 'b': 2, 'c': 3}, 'file_ending': '.nii.gz', 'channel_names': {'0': 'CT'}}


def _blobs(seed: int, top: int = 3) -> np.ndarray:
    """A label map of SHAPE: boxes of the labels 1 .. 3 on background, several components per label (``top``: label 3's value)."""
    rng = np.random.default_rng(seed)
    seg = np.zeros(SHAPE, np.uint16 if top > 255 else np.uint8)
    for k in range(12):
        lo = [int(rng.integers(0, s - 4)) for s in SHAPE]
        hi = [int(l + rng.integers(2, 9)) for l in lo]
        seg[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = (1, 2, top)[k % 3]
    return seg


def _same_maps(a, b):
    (la, pa), (lb, pb) = a, b
    assert la.dtype == lb.dtype and la.shape == lb.shape and torch.equal(la, lb)
    assert pa['spacing'] == pb['spacing'] and sorted(pa['nibabel_stuff']) == sorted(pb['nibabel_stuff'])
    for k in pa['nibabel_stuff']:
        assert np.array_equal(pa['nibabel_stuff'][k], pb['nibabel_stuff'][k])


def _device_written(rw, seg: np.ndarray, affine, folder, stem: str, mask_labels=()):
    """``seg`` as a zlib-made file, then - read with ``rw`` and compressed on the device - as a label file and as mask files."""
    from fast_nnunet_amd import imageio
    os.makedirs(folder, exist_ok=True)
    host = os.path.join(folder, stem + '_host.nii.gz')
    imageio.write_label_file(seg, host, affine)
    labels, props = rw.read_label_map(host)
    dev = os.path.join(folder, stem + '.nii.gz')
    rw.write_seg(rw.compress_labels(labels, props), dev, props)
    assert gzip.decompress(open(dev, 'rb').read()) == gzip.decompress(open(host, 'rb').read())
    masks = []
    for label, m in zip(mask_labels, rw.compress_label_masks(labels, mask_labels, props) if mask_labels else ()):
        masks.append(os.path.join(folder, f'{stem}_mask{label}.nii.gz'))
        rw.write_seg(m, masks[-1], props)
    return host, dev, masks


@pytest.mark.parametrize('reader,affine', [('NiftiIO', RAS), ('NiftiReorientIO', NOT_RAS)])
@pytest.mark.parametrize('top', [3, 300])
def test_device_written_files_read_back_on_the_device(reader, affine, top, tmp_path):
    from fast_nnunet_amd import imageio
    cls = getattr(imageio, reader)
    off, on = cls(), cls(inflate_on_device=True)
    assert off.inflate_on_device is False and on.inflate_on_device is True
    host, dev, masks = _device_written(off, _blobs(1, top), affine, str(tmp_path), 'case', mask_labels=[2, 9])   # 9: absent
    for n, f in enumerate([dev] + masks):
        _same_maps(on.read_label_map(f), off.read_label_map(f))
        assert on.inflate_stats == {'device': n + 1, 'host': 0, 'fallback': 0}
    # files zlib wrote go the host's way through the same instance
    golden = os.path.join(GOLDEN, 'example_ct_sm_T300_output.nii.gz')
    for n, f in enumerate([host, golden]):
        _same_maps(on.read_label_map(f), off.read_label_map(f))
        assert on.inflate_stats == {'device': 3, 'host': n + 1, 'fallback': 0}
    assert off.inflate_stats == {'device': 0, 'host': 5 + 1, 'fallback': 0}             # (+ 1: _device_written's own read)
    labels, _ = on.read_label_map(dev, on_device=False)                                   # the numpy route is untouched
    assert np.array_equal(labels, off.read_label_map(dev)[0].cpu().numpy().view(labels.dtype)) and on.inflate_stats['device'] == 3


BIG_SHAPE = (200, 192, 192)                                      # 7 MiB: more than the header read inflates of a file, see below


@pytest.fixture(scope='module')
def big_device_written_file(tmp_path_factory):
    from fast_nnunet_amd import imageio
    seg = np.zeros(BIG_SHAPE, np.uint8)
    rng = np.random.default_rng(5)
    for k in range(60):
        lo = [int(rng.integers(0, s - 40)) for s in BIG_SHAPE]
        seg[lo[0]:lo[0] + int(rng.integers(5, 40)), lo[1]:lo[1] + int(rng.integers(5, 40)), lo[2]:lo[2] + int(rng.integers(5, 40))] = 1 + k % 5
    _, dev, _ = _device_written(imageio.NiftiIO(), seg, RAS, str(tmp_path_factory.mktemp('big')), 'big')
    return dev


@pytest.mark.parametrize('where', [0.7, 0.8, 0.95])
def test_a_flipped_byte_falls_back_to_the_hosts_route(where, big_device_written_file, tmp_path):
    """One byte inside a chunk of a device-written file: the device route does not certify the result, the file is read
    again by zlib on the calling thread, and the call ends exactly as it ends with the flag off - the same labels, or the same
    RuntimeError.  (The byte lies behind the 4 MiB the header read inflates at the most: what lies before is inflated there,
    and refused there, before either route begins.)"""
    from fast_nnunet_amd import imageio
    off, on = imageio.NiftiIO(), imageio.NiftiIO(inflate_on_device=True)
    blob = bytearray(open(big_device_written_file, 'rb').read())
    lay = imageio.chunked_layout(bytes(blob), imageio.read_header(big_device_written_file))
    blob[lay.first + int(where * lay.in_bytes)] ^= 0x10
    bad = os.path.join(tmp_path, 'bad.nii.gz')
    with open(bad, 'wb') as f:
        f.write(blob)
    assert imageio.chunked_layout(bytes(blob), imageio.read_header(bad)) is not None

    def outcome(rw):
        try:
            labels, _ = rw.read_label_map(bad)
            return 'labels', labels.cpu().numpy().tobytes()
        except RuntimeError as e:
            return 'error', str(e)

    assert outcome(on) == outcome(off)
    assert on.inflate_stats == {'device': 0, 'host': 0, 'fallback': 1}
    _same_maps(on.read_label_map(big_device_written_file), off.read_label_map(big_device_written_file))
    assert on.inflate_stats == {'device': 1, 'host': 0, 'fallback': 1}


def _folders(tmp_path):
    from fast_nnunet_amd import imageio
    rw = imageio.NiftiIO()
    ref_dir, pred_dir = os.path.join(tmp_path, 'ref'), os.path.join(tmp_path, 'pred')
    os.makedirs(ref_dir)
    for i in range(3):
        imageio.write_label_file(_blobs(10 + i), os.path.join(ref_dir, f'c{i}.nii.gz'), RAS)
        _, dev, _ = _device_written(rw, _blobs(20 + i), RAS, os.path.join(tmp_path, 'made'), f'c{i}')
        os.makedirs(pred_dir, exist_ok=True)
        os.replace(dev, os.path.join(pred_dir, f'c{i}.nii.gz'))
    return ref_dir, pred_dir


def test_compute_metrics_on_folder_with_the_flag_on_and_off(tmp_path):
    from fast_nnunet_amd import evaluation as ev
    from fast_nnunet_amd.imageio import NiftiIO
    ref_dir, pred_dir = _folders(str(tmp_path))
    made = {}
    for flag in (False, True):
        rw = NiftiIO(inflate_on_device=flag)
        out = os.path.join(tmp_path, f'summary_{int(flag)}.json')
        made[flag] = (ev.compute_metrics_on_folder(ref_dir, pred_dir, out, rw, '.nii.gz', [1, 2, 3]), open(out).read(), rw.inflate_stats)
    assert made[True][1] == made[False][1] and json.dumps(made[True][0], default=str) == json.dumps(made[False][0], default=str)
    assert made[True][2] == {'device': 3, 'host': 3, 'fallback': 0} and made[False][2] == {'device': 0, 'host': 6, 'fallback': 0}
    assert len(made[True][0]['metric_per_case']) == 3
    for n, obj in (('plans.json', PLANS), ('dataset.json', DATASET)):
        with open(os.path.join(tmp_path, n), 'w') as f:
            json.dump(obj, f)
    for flag in (False, True):                                     # the entry that builds its own reader-writer
        ev.compute_metrics_on_folder2(ref_dir, pred_dir, os.path.join(tmp_path, 'dataset.json'), os.path.join(tmp_path, 'plans.json'),
                                      os.path.join(tmp_path, f'summary2_{int(flag)}.json'), inflate_on_device=flag)
    assert open(os.path.join(tmp_path, 'summary2_1.json')).read() == open(os.path.join(tmp_path, 'summary2_0.json')).read() == made[True][1]


def test_apply_postprocessing_to_folder_with_the_flag_on_and_off(tmp_path):
    from fast_nnunet_amd import postprocessing as pp
    _, pred_dir = _folders(str(tmp_path))
    fns, kwargs = [pp.remove_all_but_largest_component_from_segmentation], [{'labels_or_regions': [1, 2, 3]}]
    outs = {}
    for flag in (False, True):
        outs[flag] = os.path.join(tmp_path, f'out_{int(flag)}')
        pp.apply_postprocessing_to_folder(pred_dir, outs[flag], fns, kwargs, PLANS, DATASET, compress_on_device=True, inflate_on_device=flag)
    names = sorted(os.listdir(pred_dir))
    assert sorted(os.listdir(outs[True])) == sorted(os.listdir(outs[False])) == names and len(names) == 3
    changed = 0
    for n in names:
        a, b = (gzip.decompress(open(os.path.join(outs[f], n), 'rb').read()) for f in (False, True))
        assert a == b
        changed += a != gzip.decompress(open(os.path.join(pred_dir, n), 'rb').read())
    assert changed, 'the postprocessing removed something'


def test_determine_postprocessing_on_folder_with_the_flag_on_and_off(tmp_path):
    """The search reads every prediction several times through ``FolderBackend``'s prefetch, which stages with ``fill``."""
    import shutil
    from fast_nnunet_amd import postprocessing as pp
    ref_dir, pred_dir = _folders(str(tmp_path))
    made = {}
    for flag in (False, True):
        folder = os.path.join(tmp_path, f'pred_{int(flag)}')
        shutil.copytree(pred_dir, folder)
        fns, kwargs = pp.determine_postprocessing_on_folder(folder, ref_dir, PLANS, DATASET, inflate_on_device=flag)
        post = os.path.join(folder, 'postprocessed')
        files = sorted(n for n in os.listdir(post) if n.endswith('.nii.gz'))
        made[flag] = (len(fns), kwargs, open(os.path.join(folder, 'postprocessing.json')).read(),
                      [gzip.decompress(open(os.path.join(post, n), 'rb').read()) for n in files],
                      json.load(open(os.path.join(folder, 'summary.json')))['foreground_mean'])
        assert len(files) == 3
    assert made[True] == made[False]
