"""The speculative device inflate on a real MI355X: ``fnn_inflate_find_blocks`` and ``fnn_inflate_stream`` (csrc/inflate_any.hip)
against zlib byte for byte and against the Python model of the block finder, the member rule and the chain
(tests/inflate_any_ref.py) set for set and status for status, on the stream matrix of tests/inflate_any_cases.py - every
valid stream of it must be served, none may fall back - and the label-file readers and folder commands with
``inflate_on_device='any'`` against the route they take without it.

Every call runs between guard bands: 64 bytes of a pattern in front of and behind ``in`` and ``out``, which must be
unchanged afterwards.  The malformed streams here are data a decoder has to refuse with a status word - hand-made ones and a
fixed subset of the mutated corpus, all of which tests/test_inflate_any_core_host_cpu.py runs through the same rule on the
host under the sanitizers; none of them is meant to, or may, provoke a fault.
"""
import gzip
import json
import os
import zlib

import numpy as np
import pytest
import torch

import inflate_any_cases as cases
import inflate_any_ref as ref

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda', 0)
GUARD, FILL = 64, 0xA5
FIND = ['inflate_any_mark_kernel', 'inflate_any_scan_kernel', 'inflate_any_write_kernel']
KERNELS = FIND + ['inflate_any_count_kernel', 'inflate_any_emit_kernel', 'inflate_any_window_kernel', 'inflate_any_resolve_kernel']


def _stream():
    return torch.cuda.current_stream(DEV).cuda_stream


def _guarded(data: bytes, n: int = None):
    n = len(data) if n is None else n
    t = torch.full((GUARD + n + GUARD,), FILL, dtype=torch.uint8, device=DEV)
    if data:
        t[GUARD:GUARD + len(data)] = torch.frombuffer(bytearray(data), dtype=torch.uint8).to(DEV)
    assert (t.data_ptr() + GUARD) % 16 == 0
    return t


def _inflate(stream: bytes, out_bytes: int):
    """One call between guard bands -> (status, crc32, the bytes of ``out``)."""
    from fast_nnunet_amd import capi
    src, dst = _guarded(stream), _guarded(b'', out_bytes)
    before = src.cpu().numpy().copy()
    status, crc = capi.inflate_stream(src.data_ptr() + GUARD, len(stream), dst.data_ptr() + GUARD, out_bytes, _stream())
    host = dst.cpu().numpy()
    assert np.all(host[:GUARD] == FILL) and np.all(host[GUARD + out_bytes:] == FILL), 'wrote outside out[0, out_bytes)'
    assert np.array_equal(src.cpu().numpy(), before), 'the input and its guard bands are left alone'
    return status, crc, host[GUARD:GUARD + out_bytes].tobytes()


def _served(stream: bytes, data: bytes, name=''):
    from fast_nnunet_amd import capi
    status, crc, out = _inflate(stream, len(data))
    assert status == 0, (name, ref.REASONS[status])
    assert out == data, name
    assert crc == zlib.crc32(data), name
    assert capi.op_last_kernels() == (KERNELS if data else KERNELS[:4]), name


def _find(stream: bytes, cap: int = None):
    from fast_nnunet_amd import capi
    src = _guarded(stream)
    n = capi.inflate_find_blocks(src.data_ptr() + GUARD, len(stream), 0, 0, _stream())
    cap = n if cap is None else cap
    pos = torch.full((cap + 2,), -7, dtype=torch.int64, device=DEV)
    assert capi.inflate_find_blocks(src.data_ptr() + GUARD, len(stream), pos.data_ptr() + 8, cap, _stream()) == n
    assert capi.op_last_kernels() == (FIND[:3 if cap else 2] if stream else [])
    host = pos.cpu().numpy()
    assert host[0] == -7 and np.all(host[1 + min(n, cap):] == -7), 'wrote outside positions[0, min(n, cap))'
    return n, [int(p) for p in host[1:1 + min(n, cap)]]


def test_find_blocks_is_the_models_set():
    """On every stream of at most 8 KiB, the hand-made ones and 40 of the mutated corpus."""
    streams = {k: v[0] for k, v in cases.small().items()}
    streams.update({k: v[0] for k, v in cases.hand_made().items()})
    streams.update({f'mutated-{i}': s for i, (s, _) in enumerate(cases.mutated(40))})
    assert len(streams) >= 80
    found = 0
    for name, stream in streams.items():
        want = ref.find(stream)
        assert _find(stream) == (len(want), want), name
        found += len(want) - 1
    assert found >= 100, 'the streams hold dynamic blocks'
    stream = cases.matrix()['ct-65541-l6-m1'][0]                   # more than one slice, and a cap below the count
    want = ref.find(stream)
    assert len(stream) > 4096 and len(want) > 50
    assert _find(stream) == (len(want), want) and _find(stream, 7) == (len(want), want[:7])


@pytest.mark.parametrize('kind', cases.KINDS + ('own',))
def test_every_valid_stream_of_the_matrix_is_served(kind):
    """Status 0, zlib's bytes and zlib's CRC-32: no stream is left out and none may fall back."""
    names = [k for k in cases.matrix() if k.split('-')[0] == kind]
    assert len(names) >= 16
    for name in names:
        stream, data = cases.matrix()[name]
        _served(stream, data, name)


def test_required_coverage():
    """Asserted from the model's records, then served: a member longer than the ring's 32 Ki entries, runs of members
    shorter than a window, a member that runs through fixed and stored blocks, 100 cross-member matches in one stream."""
    M = cases.matrix()
    stream, data = M['runs1-300000-l6-m8']
    assert max(len(m[3]) for m in ref.inflate(stream, len(data)).members) > 2 * ref.WINDOW
    _served(stream, data)
    stream, data = M['ct-300000-l6-m1']
    r = ref.inflate(stream, len(data))
    assert sum(len(m[3]) < ref.WINDOW for m in r.members) >= 100 and sum(m[5] > 0 for m in r.members) >= 100
    types = _block_types(stream)
    assert types.count(1) > 10 and len(r.members) < len(types) - 10, 'members run through fixed blocks'
    _served(stream, data)
    stream, data = M['random-65541-l6-syncflush']
    assert 0 in _block_types(stream) and len(ref.inflate(stream, len(data)).members) < len(_block_types(stream))
    _served(stream, data)
    stream, data = M['tripled-65541-l9-m8']
    assert len(data) == 3 * 32768
    _served(stream, data)


def _block_types(stream):
    b, types = ref._Bits(bytes(stream), 0), []
    while True:
        (final, btype), _, _, _ = ref._one_block(stream, b)
        types.append(btype)
        if final:
            return types


def _like_the_model(stream: bytes, out_bytes: int, name=''):
    from fast_nnunet_amd import capi
    r = ref.inflate(stream, out_bytes)
    status, crc, out = _inflate(stream, out_bytes)
    assert ref.REASONS[status] == ref.REASONS[r.status], name
    if r.status == ref.OK:
        d = zlib.decompressobj(-15)
        assert out == d.decompress(stream) + d.flush() == r.data and crc == r.crc, name
    else:
        assert crc == 0 and capi.op_last_kernels() == KERNELS[:4], 'nothing is launched past the point of knowing'
    return r.status


def test_hand_made_and_mutated_streams_give_the_models_status():
    for name, (stream, out_bytes, status, _) in cases.hand_made().items():
        assert _like_the_model(stream, out_bytes, name) == status
    seen = {_like_the_model(s, n, i) for i, (s, n) in enumerate(cases.mutated(160))}
    assert {ref.OK, ref.END, ref.TABLES, ref.SYMBOL, ref.DISTANCE, ref.FINAL, ref.SIZE, ref.OUTPUT} <= seen, seen


def test_a_wrong_out_bytes_is_a_status_and_nothing_outside_is_written():
    for name in ('runs1-32769-l6-m1', 'ct-65541-l6-m1', 'random-255-l0', 'runs2-65541-l6-fixed', 'own-dynamic2-32769', 'runs1-1-l6-m8'):
        stream, data = cases.matrix()[name]
        for wrong in (len(data) - 1, len(data) + 1):
            assert _like_the_model(stream, wrong, name) in (ref.SIZE, ref.OUTPUT), name


def test_empty_inputs_launch_nothing():
    from fast_nnunet_amd import capi
    assert _inflate(b'', 0)[:2] == (0, 0)
    assert capi.op_last_kernels() == []
    assert _inflate(b'', 5)[:2] == (ref.SIZE, 0)
    assert _find(b'') == (0, [])
    _served(b'\x03\x00', b'')


def test_two_calls_give_identical_bytes():
    stream, data = cases.matrix()['ct-65541-l6-m1']
    first = _inflate(stream, len(data))
    assert first == _inflate(stream, len(data)) and first[2] == data


# ---------------------------------------------------------------------------------------------------------------
# files: label files that zlib wrote, read with the switch off and 'any'
# ---------------------------------------------------------------------------------------------------------------
SHAPE = (32, 40, 48)
RAS = np.diag([1.5, 2.0, 0.5, 1.0])
NOT_RAS = np.array([[0.0, -2.0, 0.0, 5.0], [1.5, 0.0, 0.0, -3.0], [0.0, 0.0, -0.5, 7.0], [0.0, 0.0, 0.0, 1.0]])
PLANS = {'dataset_name': 'd', 'plans_name': 'p', 'image_reader_writer': 'NibabelIO', 'configurations': {}}
DATASET = {'labels': {'background': 0, 'a': 1, 'b': 2, 'c': 3}, 'file_ending': '.nii.gz', 'channel_names': {'0': 'CT'}}


def _blobs(seed: int, top: int = 3, shape=SHAPE) -> np.ndarray:
    rng = np.random.default_rng(seed)
    seg = np.zeros(shape, np.uint16 if top > 255 else np.uint8)
    for k in range(12):
        lo = [int(rng.integers(0, s - 4)) for s in shape]
        hi = [int(l + rng.integers(2, 9)) for l in lo]
        seg[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = (1, 2, top)[k % 3]
    return seg


def _same_maps(a, b):
    (la, pa), (lb, pb) = a, b
    assert la.dtype == lb.dtype and la.shape == lb.shape and torch.equal(la, lb)
    assert pa['spacing'] == pb['spacing'] and sorted(pa['nibabel_stuff']) == sorted(pb['nibabel_stuff'])
    for k in pa['nibabel_stuff']:
        assert np.array_equal(pa['nibabel_stuff'][k], pb['nibabel_stuff'][k])


def _with_fname_field(src: str, dst: str):
    """The file's bytes in a gzip member whose header carries FNAME, a comment-free header of 10 + len(name) + 1 bytes."""
    with open(dst, 'wb') as f, gzip.GzipFile(filename='a_name.nii', mode='wb', fileobj=f, compresslevel=6, mtime=0) as g:
        g.write(gzip.decompress(open(src, 'rb').read()))
    assert open(dst, 'rb').read()[3] & 8


@pytest.mark.parametrize('reader,affine', [('NiftiIO', RAS), ('NiftiReorientIO', NOT_RAS)])
@pytest.mark.parametrize('top', [3, 300])
def test_files_that_zlib_wrote_are_inflated_on_the_device(reader, affine, top, tmp_path):
    from fast_nnunet_amd import imageio
    cls = getattr(imageio, reader)
    off = cls()
    host = os.path.join(tmp_path, 'host.nii.gz')
    imageio.write_label_file(_blobs(1, top), host, affine)         # the host route: compress_on_device=False
    named = os.path.join(tmp_path, 'named.nii.gz')
    _with_fname_field(host, named)
    for f in (host, named):
        rw = cls(inflate_on_device='any')
        assert rw.inflate_on_device == 'any'
        _same_maps(rw.read_label_map(f), off.read_label_map(f))
        assert rw.inflate_stats == {'device': 1, 'host': 0, 'fallback': 0}, f
    # what the other values of the switch do with such a file is what they did
    for flag in (True, 'dynamic'):
        rw = cls(inflate_on_device=flag)
        _same_maps(rw.read_label_map(host), off.read_label_map(host))
        assert rw.inflate_stats == {'device': 0, 'host': 1, 'fallback': 0}
    # the project's own files keep the segment route
    rw = cls(inflate_on_device='any')
    labels, props = off.read_label_map(host)
    own = os.path.join(tmp_path, 'own.nii.gz')
    off.write_seg(off.compress_labels(labels, props, tables='dynamic'), own, props)
    _same_maps(rw.read_label_map(own), off.read_label_map(own))
    assert rw.inflate_stats == {'device': 1, 'host': 0, 'fallback': 0}
    assert rw.stage_label_files([own]).fill().layouts[0].starts is not None and rw.stage_label_files([host]).fill().layouts[0].starts is None
    with pytest.raises(ValueError, match='inflate_on_device'):
        cls(inflate_on_device='Any')


def test_multi_member_files_trailing_bytes_and_odd_headers_go_to_the_host(tmp_path):
    from fast_nnunet_amd import imageio
    off, rw = imageio.NiftiIO(), imageio.NiftiIO(inflate_on_device='any')
    host = os.path.join(tmp_path, 'host.nii.gz')
    imageio.write_label_file(_blobs(2), host, RAS)
    whole = gzip.decompress(open(host, 'rb').read())
    two, trailing = os.path.join(tmp_path, 'two.nii.gz'), os.path.join(tmp_path, 'trailing.nii.gz')
    with open(two, 'wb') as f:
        f.write(gzip.compress(whole[:5000], mtime=0) + gzip.compress(whole[5000:], mtime=0))
    with open(trailing, 'wb') as f:
        f.write(open(host, 'rb').read() + bytes(5))

    def outcome(r, fname):
        try:
            labels, _ = r.read_label_map(fname)
            return 'labels', labels.cpu().numpy().tobytes()
        except (RuntimeError, zlib.error, OSError) as e:
            return type(e).__name__, str(e)

    for n, f in enumerate((two, trailing)):                        # ISIZE is not where, or what, a single member has it
        assert imageio.stream_layout(open(f, 'rb').read(), imageio.read_header(f)) is None
        assert outcome(rw, f) == outcome(off, f)
        assert rw.inflate_stats['device'] == rw.inflate_stats['fallback'] == 0
    blob = open(host, 'rb').read()
    assert imageio.gzip_member_start(blob) == 10 and imageio.gzip_member_start(blob[:3] + b'\x04\x00\x00\x00\x00\x00\x03\x05\x00' + blob[10:]) == 17
    assert imageio.gzip_member_start(blob[:3] + b'\x20' + blob[4:]) is None and imageio.gzip_member_start(blob[:3] + b'\x08' + b'\x01' * 40) is None


def test_a_flipped_bit_falls_back_to_the_hosts_route(tmp_path):
    """One bit of the deflate stream behind the 4 MiB that the header read inflates at the most: the device route does not
    certify the result, the file is read again by zlib on the calling thread, and the call ends exactly as it ends with the
    switch off."""
    from fast_nnunet_amd import imageio
    seg = _blobs(5, shape=(128, 256, 256))
    rng = np.random.default_rng(5)
    for k in range(60):
        lo = [int(rng.integers(0, s - 40)) for s in seg.shape]
        seg[lo[0]:lo[0] + int(rng.integers(5, 40)), lo[1]:lo[1] + int(rng.integers(5, 40)), lo[2]:lo[2] + int(rng.integers(5, 40))] = 1 + k % 5
    off, rw = imageio.NiftiIO(), imageio.NiftiIO(inflate_on_device='any')
    good = os.path.join(tmp_path, 'good.nii.gz')
    imageio.write_label_file(seg, good, RAS)
    blob = bytearray(open(good, 'rb').read())
    d = zlib.decompressobj(-15)
    assert len(d.decompress(bytes(blob[10:len(blob) * 9 // 10]))) > 5 << 20, 'the flip lies behind the header read'
    blob[len(blob) * 19 // 20] ^= 0x10
    bad = os.path.join(tmp_path, 'bad.nii.gz')
    with open(bad, 'wb') as f:
        f.write(blob)

    def outcome(r):
        try:
            labels, _ = r.read_label_map(bad)
            return 'labels', labels.cpu().numpy().tobytes()
        except (RuntimeError, zlib.error, OSError) as e:
            return type(e).__name__, str(e)

    assert outcome(rw) == outcome(off)
    assert rw.inflate_stats == {'device': 0, 'host': 0, 'fallback': 1}
    _same_maps(rw.read_label_map(good), off.read_label_map(good))
    assert rw.inflate_stats == {'device': 1, 'host': 0, 'fallback': 1}


def _folders(tmp_path):
    from fast_nnunet_amd import imageio
    ref_dir, pred_dir = os.path.join(tmp_path, 'ref'), os.path.join(tmp_path, 'pred')
    os.makedirs(ref_dir)
    os.makedirs(pred_dir)
    for i in range(2):
        imageio.write_label_file(_blobs(10 + i), os.path.join(ref_dir, f'c{i}.nii.gz'), RAS)
        imageio.write_label_file(_blobs(20 + i), os.path.join(pred_dir, f'c{i}.nii.gz'), RAS)
    return ref_dir, pred_dir


def test_compute_metrics_on_folder_with_the_switch_off_and_any(tmp_path):
    from fast_nnunet_amd import evaluation as ev
    from fast_nnunet_amd.imageio import NiftiIO
    ref_dir, pred_dir = _folders(str(tmp_path))
    made = {}
    for flag in (False, 'any'):
        rw = NiftiIO(inflate_on_device=flag)
        out = os.path.join(tmp_path, f'summary_{flag}.json')
        made[flag] = (ev.compute_metrics_on_folder(ref_dir, pred_dir, out, rw, '.nii.gz', [1, 2, 3]), open(out).read(), rw.inflate_stats)
    assert made['any'][1] == made[False][1] and json.dumps(made['any'][0], default=str) == json.dumps(made[False][0], default=str)
    assert made['any'][2] == {'device': 4, 'host': 0, 'fallback': 0} and made[False][2] == {'device': 0, 'host': 4, 'fallback': 0}
    for n, obj in (('plans.json', PLANS), ('dataset.json', DATASET)):
        with open(os.path.join(tmp_path, n), 'w') as f:
            json.dump(obj, f)
    for flag in (False, 'any'):                                    # the entry that builds its own reader-writer
        ev.compute_metrics_on_folder2(ref_dir, pred_dir, os.path.join(tmp_path, 'dataset.json'), os.path.join(tmp_path, 'plans.json'),
                                      os.path.join(tmp_path, f'summary2_{flag}.json'), inflate_on_device=flag)
    assert open(os.path.join(tmp_path, 'summary2_any.json')).read() == open(os.path.join(tmp_path, 'summary2_False.json')).read() == made[False][1]


def test_apply_postprocessing_to_folder_with_the_switch_off_and_any(tmp_path):
    from fast_nnunet_amd import postprocessing as pp
    _, pred_dir = _folders(str(tmp_path))
    fns, kwargs = [pp.remove_all_but_largest_component_from_segmentation], [{'labels_or_regions': [1, 2, 3]}]
    outs = {}
    for flag in (False, 'any'):
        outs[flag] = os.path.join(tmp_path, f'out_{flag}')
        pp.apply_postprocessing_to_folder(pred_dir, outs[flag], fns, kwargs, PLANS, DATASET, inflate_on_device=flag)
    names = sorted(os.listdir(pred_dir))
    assert sorted(os.listdir(outs['any'])) == sorted(os.listdir(outs[False])) == names and len(names) == 2
    changed = 0
    for n in names:
        a, b = (open(os.path.join(outs[f], n), 'rb').read() for f in (False, 'any'))
        assert a == b
        changed += gzip.decompress(a) != gzip.decompress(open(os.path.join(pred_dir, n), 'rb').read())
    assert changed, 'the postprocessing removed something'
