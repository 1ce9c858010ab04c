"""Label files on a real MI355X: ``fnn_decode_labels`` against the numpy restatement tests/label_files_ref.py (labels, flags,
maximum, nothing written outside ``out``), ``read_label_map`` with reorientation against tests/orient_ref.py, and the four
folder front-ends against the golden data the reference made (tests/golden/evaluation.*, ensemble.npz) and against the
array functions they are built on.  Every comparison is exact.

Kernels launched here (csrc/imageio.hip): decode_labels_kernel<T, OB> for T in unsigned char, signed char, short, unsigned
short, int, unsigned int, float, double and OB in 1, 2 - each with and without the shifted body, with no body at all and with
edges on both sides.
"""
import gzip
import json
import os
import pickle
import threading
from fractions import Fraction

import numpy as np
import pytest
import torch

import label_files_ref as lref
import nifti_ref
import orient_ref
from evaluation_ref import dataset_maps, load_golden, same, type_tree, untyped

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda', 0)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
CODES = sorted(lref.NIFTI_CODES)
N_VOX = (0, 1, 3, 15, 16, 17, 63, 64, 65, 4099)
GUARD, FILL = 32, 0xA5
META, ARRAYS = load_golden()
DATASETS = sorted(META)
PLANS = {'dataset_name': 'd', 'plans_name': 'p', 'image_reader_writer': 'NibabelIO', 'configurations': {}}


# ---------------------------------------------------------------------------------------------------------------
# fnn_decode_labels
# ---------------------------------------------------------------------------------------------------------------
def _values(code, n, seed):
    """n stored values: mostly labels, and every kind of voxel that is none."""
    rng = np.random.default_rng(1000 * code + seed)
    dt = np.dtype(lref.NIFTI_CODES[code])
    v = rng.integers(0, 120, n).astype(np.float64)
    if dt.itemsize > 1:
        wide = rng.random(n) < 0.1
        v[wide] = rng.integers(256, 32768 if dt == np.int16 else 65536, int(wide.sum()))
    bad = rng.random(n) < 0.08
    pool = [255, 254]
    if dt.kind == 'i':
        pool += [-1, -128]
    if dt.itemsize > 1:
        pool += [256, 257, 32767]
    if dt.itemsize > 2:
        pool += [65535, 65536, 2 ** 24 + 1, 2 ** 31 - 1 if dt.kind != 'u' else 2 ** 32 - 1]
        if dt.kind in 'if':
            pool += [-65536, -(2 ** 24 + 1)]
    if dt.kind == 'f':
        pool += [0.5, 1.5, -0.5, -0.0, np.nan, np.inf, -np.inf, 65535.5, 255.00002, 1e30, -1e30, 2.0 ** -149]
    v[bad] = rng.choice(np.array(pool, dtype=np.float64), int(bad.sum()))
    with np.errstate(invalid='ignore'):
        return v.astype(dt)


def _launch_all_offsets(capi, raw, code, swap, n, scale, slope, inter, ob):
    """One launch per byte offset of ``out`` (every element-aligned one of 0..15) into one guarded buffer -> per offset
    (labels, bytes before, bytes behind, status)."""
    offsets = list(range(0, 16, ob))
    region = GUARD + 16 + n * ob + GUARD
    region += -region % 16
    buf = torch.full((region * len(offsets),), FILL, dtype=torch.uint8, device=DEV)
    status = torch.full((len(offsets), 2), -7, dtype=torch.int32, device=DEV)
    assert buf.data_ptr() % 16 == 0
    stream = torch.cuda.current_stream(DEV).cuda_stream
    for k, off in enumerate(offsets):
        capi.decode_labels(raw.data_ptr(), code, swap, n, scale, slope, inter, ob, buf.data_ptr() + k * region + GUARD + off,
                           status[k].data_ptr(), stream)
    host, said = buf.cpu().numpy(), status.cpu().numpy()
    out = []
    for k, off in enumerate(offsets):
        r = host[k * region:(k + 1) * region]
        lo = GUARD + off
        out.append((off, r[lo:lo + n * ob].view(lref.OUT_DTYPE[ob]), r[:lo], r[lo + n * ob:], said[k]))
    return out


@pytest.mark.parametrize('ob', [1, 2], ids=['uint8', 'uint16'])
@pytest.mark.parametrize('code', CODES, ids=[lref.NIFTI_CODES[c] for c in CODES])
def test_decode_labels_equals_the_restatement(code, ob):
    from fast_nnunet_amd import capi
    launches = 0
    for n in N_VOX:
        v = _values(code, n, n)
        for swap in (0, 1):
            raw_host = (v.byteswap() if swap else v).tobytes()
            raw = torch.frombuffer(bytearray(raw_host + b'\0' * 16), dtype=torch.uint8).to(DEV)
            assert raw.data_ptr() % 16 == 0
            for scale, slope, inter in ((0, 1.0, 0.0), (1, 2.0, 1.0), (1, 0.5, 0.0)):
                want, flags, top = lref.judge(v, scale, slope, inter, ob)
                for off, got, before, behind, said in _launch_all_offsets(capi, raw, code, swap, n, scale, slope, inter, ob):
                    where = (lref.NIFTI_CODES[code], ob, n, swap, scale, slope, off)
                    assert np.all(before == FILL) and np.all(behind == FILL), (where, 'wrote outside out[0, n_vox * out_bytes)')
                    if not np.array_equal(got, want):
                        i = int(np.flatnonzero(got != want)[0])
                        raise AssertionError(f'{where}: voxel {i} (stored {v[i]!r}) is {got[i]}, the restatement says {want[i]}; '
                                             f'{int((got != want).sum())} of {n} differ')
                    assert (int(said[0]), int(said[1])) == (flags, top), (where, said, flags, top)
                    launches += 1
    assert launches == len(N_VOX) * 2 * 3 * (16 // ob)


FLAG_CASES = {
    # name: (datatype code, out bytes, offending stored value, its flag)
    'fraction_f32': (16, 2, 1.5, lref.NOT_INTEGRAL),
    'nan_f32': (16, 2, np.nan, lref.NOT_INTEGRAL),
    'negative_i16': (4, 2, -1, lref.NEGATIVE),
    'above_uint8': (4, 1, 256, lref.TOO_LARGE),
    'above_uint16_i32': (8, 2, 65536, lref.TOO_LARGE),
}


@pytest.mark.parametrize('place', ['first', 'last', 'body', 'head', 'tail'])
@pytest.mark.parametrize('case', sorted(FLAG_CASES))
def test_one_offending_voxel_gives_exactly_its_flag(case, place):
    from fast_nnunet_amd import capi
    code, ob, value, flag = FLAG_CASES[case]
    n, off = 4099, 3 * ob                                        # out starts 3 elements past a 16-byte boundary: a head of 16 / ob - 3
    head = 16 // ob - 3
    at = {'first': 0, 'last': n - 1, 'body': 2000, 'head': head - 1, 'tail': n - 3}[place]
    assert (place != 'head' or 0 < at < head) and (place != 'body' or head < at < n - 64)
    v = (np.arange(n) * 5 % 97).astype(lref.NIFTI_CODES[code])
    v[at] = value
    want, flags, top = lref.judge(v, 0, 1.0, 0.0, ob)
    assert flags == flag and want[at] == 0 and np.array_equal(np.delete(want, at), np.delete(v, at).astype(want.dtype))
    raw = torch.frombuffer(bytearray(v.tobytes()), dtype=torch.uint8).to(DEV)
    buf = torch.full((GUARD + 16 + n * ob + GUARD,), FILL, dtype=torch.uint8, device=DEV)
    status = torch.full((2,), -7, dtype=torch.int32, device=DEV)
    capi.decode_labels(raw.data_ptr(), code, 0, n, 0, 1.0, 0.0, ob, buf.data_ptr() + GUARD + off, status.data_ptr(),
                       torch.cuda.current_stream(DEV).cuda_stream)
    host = buf.cpu().numpy()
    got = host[GUARD + off:GUARD + off + n * ob].view(lref.OUT_DTYPE[ob])
    assert status.tolist() == [flag, top] and top == 96
    assert got[at] == 0 and np.array_equal(got, want)
    assert np.all(host[:GUARD + off] == FILL) and np.all(host[GUARD + off + n * ob:] == FILL)


def test_two_conditions_give_the_or_of_their_flags():
    from fast_nnunet_amd import capi
    n = 4099
    v = (np.arange(n) * 5 % 97).astype(np.float32)
    v[7], v[3000] = -2.0, 2.5
    want, flags, top = lref.judge(v, 0, 1.0, 0.0, 1)
    assert flags == lref.NEGATIVE | lref.NOT_INTEGRAL
    raw = torch.frombuffer(bytearray(v.tobytes()), dtype=torch.uint8).to(DEV)
    out = torch.full((n,), FILL, dtype=torch.uint8, device=DEV)
    status = torch.full((2,), -7, dtype=torch.int32, device=DEV)
    for _ in range(3):                                           # (the same on every run)
        capi.decode_labels(raw.data_ptr(), 16, 0, n, 0, 1.0, 0.0, 1, out.data_ptr(), status.data_ptr(),
                           torch.cuda.current_stream(DEV).cuda_stream)
        assert status.tolist() == [flags, top] and np.array_equal(out.cpu().numpy(), want)


def test_decode_labels_refuses_what_it_cannot_serve():
    from fast_nnunet_amd import capi
    raw = torch.zeros(64, dtype=torch.uint8, device=DEV)
    out = torch.full((64,), FILL, dtype=torch.uint8, device=DEV)
    status = torch.full((2,), -7, dtype=torch.int32, device=DEV)
    args = dict(byteswap=0, n_vox=4, scale=0, slope=1.0, inter=0.0)
    with pytest.raises(AssertionError, match='16-byte aligned'):
        capi.decode_labels(raw.data_ptr() + 4, 2, out_bytes=1, out_ptr=out.data_ptr(), status_ptr=status.data_ptr(), **args)
    with pytest.raises(AssertionError, match='aligned to its element'):
        capi.decode_labels(raw.data_ptr(), 2, out_bytes=2, out_ptr=out.data_ptr() + 1, status_ptr=status.data_ptr(), **args)
    with pytest.raises(AssertionError, match='out_bytes'):
        capi.decode_labels(raw.data_ptr(), 2, out_bytes=4, out_ptr=out.data_ptr(), status_ptr=status.data_ptr(), **args)
    with pytest.raises(NotImplementedError, match='datatype'):
        capi.decode_labels(raw.data_ptr(), 1024, out_bytes=1, out_ptr=out.data_ptr(), status_ptr=status.data_ptr(), **args)
    with pytest.raises(AssertionError, match='device pointers'):
        capi.decode_labels(raw.data_ptr(), 2, out_bytes=1, out_ptr=out.cpu().data_ptr(), status_ptr=status.data_ptr(), **args)
    torch.cuda.synchronize()
    assert bool((out == FILL).all()) and status.tolist() == [-7, -7]


# ---- scaling: two roundings, not one
def _f32_of_fraction(x):
    """x rounded ONCE to float32 (nearest, ties to even)."""
    f = np.float32(float(x))
    best = None
    for c in (f, np.nextafter(f, np.float32(np.inf)), np.nextafter(f, np.float32(-np.inf))):
        key = (abs(Fraction(float(c)) - x), int(np.float32(c).view(np.uint32)) & 1)
        if best is None or key < best[0]:
            best = (key, c)
    return best[1]


def _fused_label_inputs(slope, inter):
    """float64 stored values for which the value rule's two roundings and a fused multiply-add's single one end in
    different float32 values of which one is a label: searched next to the float32 ties around small integers."""
    found = []
    for n in range(1, 10):
        below = float(np.float32(n) - np.nextafter(np.float32(n), np.float32(0)))
        for tie in (n + float(np.spacing(np.float32(n))) / 2, n - below / 2):
            x = np.float64((tie - inter) / slope)
            for _ in range(300):
                x = np.nextafter(x, -np.inf)
            for _ in range(600):
                two = np.float32(np.float64(x) * np.float64(slope) + np.float64(inter))
                single = _f32_of_fraction(Fraction(float(x)) * Fraction(slope) + Fraction(inter))
                if two != single and (two == np.trunc(two) or single == np.trunc(single)):
                    found.append((float(x), float(two), float(single)))
                x = np.nextafter(x, np.inf)
    return found


def test_scaling_is_two_roundings_where_a_fused_multiply_add_says_otherwise():
    from fast_nnunet_amd import capi
    from test_gpu_imageio import _fused_pair
    slope, inter, _ = _fused_pair()
    found = _fused_label_inputs(slope, inter)
    if not found:
        pytest.skip(f'no label-valued input on which slope {slope!r}, intercept {inter!r} tell a fused multiply-add from two roundings')
    v = np.array([f[0] for f in found], dtype=np.float64)
    for ob in (1, 2):
        want, flags, top = lref.judge(v, 1, slope, inter, ob)
        fused = np.array([f[2] for f in found], dtype=np.float32)
        fused_labels, fused_flags, _ = lref.file_labels(fused, ob)
        differ = (want != fused_labels) | ((want == 0) != (fused_labels == 0))
        assert differ.any()
        for swap in (0, 1):
            raw = torch.frombuffer(bytearray((v.byteswap() if swap else v).tobytes()), dtype=torch.uint8).to(DEV)
            for off, got, before, behind, said in _launch_all_offsets(capi, raw, 64, swap, v.size, 1, slope, inter, ob):
                assert np.array_equal(got, want), (ob, swap, off, np.flatnonzero(got != want)[:5])
                assert (int(said[0]), int(said[1])) == (flags, top)
                assert np.all(before == FILL) and np.all(behind == FILL)


# ---------------------------------------------------------------------------------------------------------------
# read_label_map
# ---------------------------------------------------------------------------------------------------------------
ORIENTATIONS = {'flip': ((0, 1, 2), (-1, 1, 1)), 'swap_fastest': ((1, 0, 2), (1, 1, 1)), 'both': ((2, 0, 1), (1, -1, -1))}


@pytest.mark.parametrize('code', [2, 4], ids=['uint8_file', 'int16_file'])
@pytest.mark.parametrize('name', sorted(ORIENTATIONS))
def test_reoriented_label_map_equals_the_host_route(name, code, tmp_path):
    from fast_nnunet_amd.imageio import NiftiIO, NiftiReorientIO
    perm, signs = ORIENTATIONS[name]
    affine = orient_ref.affine_of(perm, signs)
    seg = (np.arange(5 * 6 * 7) * 11 % 23).reshape(5, 6, 7)
    if code == 4:
        seg[1, 2, 3] = 300                                       # a map that stays two bytes wide
    fname = os.path.join(tmp_path, 'seg.nii.gz')
    nifti_ref.write(fname, seg, code, sform=affine[:3], sform_code=1, pixdim=(1, *orient_ref.ZOOMS))
    values, info = nifti_ref.read(fname)
    want, _ = orient_ref.to_ras(values, info['affine'])
    rw = NiftiReorientIO()
    got, props = rw.read_label_map(fname)
    assert got.device.type == 'cuda' and got.dtype == (torch.int16 if code == 4 else torch.uint8)
    assert tuple(got.shape) == want.shape and (name == 'flip' or want.shape != seg.shape)
    assert np.array_equal(got.cpu().numpy().astype(np.int64), want.astype(np.int64))
    host, props_h = rw.read_label_map(fname, on_device=False)
    assert np.array_equal(host, want.astype(host.dtype)) and host.dtype == (np.uint16 if code == 4 else np.uint8)
    _, props_i = rw.read_images([fname])
    for p in (props, props_h):
        assert p.keys() == props_i.keys() and p['spacing'] == props_i['spacing']
        for k in ('original_affine', 'reoriented_affine'):
            assert np.array_equal(p['nibabel_stuff'][k], props_i['nibabel_stuff'][k])
    plain, _ = NiftiIO().read_label_map(fname)
    assert np.array_equal(plain.cpu().numpy(), seg.astype(np.int64))


def test_read_label_map_names_the_file_and_the_condition(tmp_path):
    from fast_nnunet_amd.imageio import NiftiIO
    for case, (code, value, said) in {'fraction': (16, 0.25, 'not integral'), 'negative': (256, -4, 'negative'),
                                      'above': (768, 70000, 'above 65535')}.items():
        v = np.ones((3, 4, 5), lref.NIFTI_CODES[code])
        v[2, 3, 4] = value
        fname = os.path.join(tmp_path, case + '.nii')
        nifti_ref.write(fname, v, code, order='>')
        for on_device in (True, False):
            with pytest.raises(RuntimeError, match=said) as e:
                NiftiIO().read_label_map(fname, on_device=on_device)
            assert fname in str(e.value)


# ---------------------------------------------------------------------------------------------------------------
# folders
# ---------------------------------------------------------------------------------------------------------------
AFFINE = np.array([[-1.5, 0, 0, 10.0], [0, 2.0, 0, -20.5], [0, 0, 0.5, 3.0], [0, 0, 0, 1.0]])
PRED_TYPES = [(4, '<'), (768, '>'), (2, '<'), (8, '<'), (512, '>')]           # (datatype, byte order) of case i's prediction


def _write_maps(folder, names, maps, types, affine=AFFINE):
    os.makedirs(folder, exist_ok=True)
    files = []
    for i, (n, m) in enumerate(zip(names, maps)):
        code, order = types[i % len(types)]
        files.append(os.path.join(folder, n + '.nii.gz'))
        nifti_ref.write(files[-1], m, code, order=order, sform=affine[:3], sform_code=1,
                        pixdim=(1, *np.sqrt((affine[:3, :3] ** 2).sum(0))))
    return files


def _golden_folders(tmp_path, name):
    names, refs, preds = dataset_maps(META, ARRAYS, name)
    # references and predictions of different integer datatypes: 1-byte maps, 2-byte maps narrowed to uint8, both byte orders
    files_ref = _write_maps(os.path.join(tmp_path, 'ref'), names, refs, [(2, '<'), (4, '>')])
    files_pred = _write_maps(os.path.join(tmp_path, 'pred'), names, preds, PRED_TYPES)
    dj = dict(META[name]['dataset_json'], file_ending='.nii.gz')
    return names, refs, preds, files_ref, files_pred, dj


def _labels_or_regions(dj):
    from fast_nnunet_amd.plans import LabelManager
    lm = LabelManager(dj['labels'], dj.get('regions_class_order'))
    return lm, (list(lm.foreground_regions) if lm.has_regions else [np.int64(v) for v in lm.foreground_labels])


def _key(k):
    return int(k) if '(' not in k else tuple(int(p) for p in k.strip('()').split(',') if p.strip())


def _with_paths(summary, files_ref, files_pred):
    out = json.loads(json.dumps(summary))
    assert len(out['metric_per_case']) == len(files_pred)
    for case, r, p in zip(out['metric_per_case'], files_ref, files_pred):
        case['reference_file'], case['prediction_file'] = r, p
    return out


def _file_labels(fname):
    blob = nifti_ref.file_bytes(fname)
    values, info = nifti_ref.read(fname)
    return values, info, blob


@pytest.mark.parametrize('name', DATASETS)
def test_compute_metrics_on_folder_equals_the_reference_summary(name, tmp_path):
    from fast_nnunet_amd import evaluation as ev
    from fast_nnunet_amd.imageio import NiftiIO
    names, refs, preds, files_ref, files_pred, dj = _golden_folders(tmp_path, name)
    lm, lor = _labels_or_regions(dj)
    out = os.path.join(tmp_path, 'pred', 'summary.json')
    got = ev.compute_metrics_on_folder(os.path.join(tmp_path, 'ref'), os.path.join(tmp_path, 'pred'), out, NiftiIO(), '.nii.gz',
                                       lor, lm.ignore_label)
    want_json = _with_paths(META[name]['baseline_summary'], files_ref, files_pred)
    with open(out) as f:
        assert same(json.load(f), want_json)
    want = dict(want_json, mean={_key(k): v for k, v in want_json['mean'].items()})
    for case in want['metric_per_case']:
        case['metrics'] = {_key(k): v for k, v in case['metrics'].items()}
    assert same(got, want)
    assert [c['prediction_file'] for c in got['metric_per_case']] == files_pred
    assert [c['reference_file'] for c in got['metric_per_case']] == files_ref
    assert same(ev.load_summary_json(out), got)


def test_a_pair_of_different_shapes_names_both_files(tmp_path):
    from fast_nnunet_amd import evaluation as ev
    from fast_nnunet_amd.imageio import NiftiIO
    r = _write_maps(os.path.join(tmp_path, 'ref'), ['a'], [np.ones((4, 5, 6))], [(2, '<')])
    p = _write_maps(os.path.join(tmp_path, 'pred'), ['a'], [np.ones((4, 6, 5))], [(2, '<')])
    with pytest.raises(ValueError) as e:
        ev.compute_metrics_on_folder(os.path.join(tmp_path, 'ref'), os.path.join(tmp_path, 'pred'), None, NiftiIO(), '.nii.gz', [1])
    assert r[0] in str(e.value) and p[0] in str(e.value)
    assert not [t.name for t in threading.enumerate() if t.name.startswith('fnn-')]


@pytest.mark.parametrize('name', DATASETS)
def test_determine_postprocessing_on_folder_equals_golden(name, tmp_path):
    from fast_nnunet_amd import postprocessing as pp
    names, refs, preds, files_ref, files_pred, dj = _golden_folders(tmp_path, name)
    folder_pred, folder_ref = os.path.join(tmp_path, 'pred'), os.path.join(tmp_path, 'ref')
    fns, kwargs = pp.determine_postprocessing_on_folder(folder_pred, folder_ref, PLANS, dj)
    want, want_types = untyped(META[name]['kwargs'])
    assert kwargs == want and type_tree(kwargs) == want_types
    assert len(fns) == len(META[name]['pp_fns']) and all(f is pp.remove_all_but_largest_component_from_segmentation for f in fns)
    with open(os.path.join(folder_pred, 'postprocessing.json')) as f:
        assert same(json.load(f), META[name]['postprocessing_json'])
    with open(os.path.join(folder_pred, 'summary.json')) as f:
        assert same(json.load(f), _with_paths(META[name]['baseline_summary'], files_ref, files_pred))
    post = os.path.join(folder_pred, 'postprocessed')
    assert sorted(os.listdir(post)) == sorted([n + '.nii.gz' for n in names] + ['summary.json'])
    with open(os.path.join(post, 'summary.json')) as f:
        final = json.load(f)
    assert same(final['mean'], META[name]['final_summary']['mean'])
    assert same(final['foreground_mean'], META[name]['final_summary']['foreground_mean'])
    for n, src in zip(names, files_pred):
        values, info, _ = _file_labels(os.path.join(post, n + '.nii.gz'))
        assert np.array_equal(values, ARRAYS[f'{name}__{n}__postprocessed'])
        assert np.array_equal(info['affine'], nifti_ref.read(src)[1]['affine'])
    fns2, kws2 = pp.load_postprocessing_pkl(os.path.join(folder_pred, 'postprocessing.pkl'))
    pkl_want, pkl_types = untyped(META[name]['pkl_kwargs'])
    assert kws2 == pkl_want and type_tree(kws2) == pkl_types
    assert not os.path.exists(os.path.join(post, 'temp'))
    assert not [i for i in os.listdir(folder_pred) + os.listdir(post) if '.part' in i]
    # once more without the files: the summary.json of the first run is reused, and no folder is left
    import shutil
    shutil.rmtree(post)
    os.remove(os.path.join(folder_pred, 'postprocessing.json'))
    stamp = os.stat(os.path.join(folder_pred, 'summary.json')).st_mtime_ns
    fns3, kwargs3 = pp.determine_postprocessing_on_folder(folder_pred, folder_ref, PLANS, dj, keep_postprocessed_files=False)
    assert kwargs3 == want and type_tree(kwargs3) == want_types and len(fns3) == len(fns)
    assert not os.path.exists(post) and os.stat(os.path.join(folder_pred, 'summary.json')).st_mtime_ns == stamp
    with open(os.path.join(folder_pred, 'postprocessing.json')) as f:
        assert same(json.load(f), META[name]['postprocessing_json'])
    assert not [t.name for t in threading.enumerate() if t.name.startswith('fnn-')]


@pytest.mark.parametrize('reader', ['NibabelIO', 'NibabelIOWithReorient'])
@pytest.mark.parametrize('name', ['labels_mixed', 'regions'])
def test_apply_postprocessing_to_folder_equals_the_array_route(name, reader, tmp_path):
    from fast_nnunet_amd import postprocessing as pp
    names, refs, preds, _, files_pred, dj = _golden_folders(tmp_path, name)
    kwargs, _ = untyped(META[name]['pkl_kwargs'])
    fns = [pp.remove_all_but_largest_component_from_segmentation] * len(kwargs)
    plans = dict(PLANS, image_reader_writer=reader)
    folder_pred = os.path.join(tmp_path, 'pred')
    for n, obj in (('plans.json', plans), ('dataset.json', dj)):
        with open(os.path.join(folder_pred, n), 'w') as f:
            json.dump(obj, f)
    out_a, out_b = os.path.join(tmp_path, 'out_host'), os.path.join(tmp_path, 'out_device')
    pp.apply_postprocessing_to_folder(folder_pred, out_a, fns, kwargs)
    pp.apply_postprocessing_to_folder(folder_pred, out_b, fns, kwargs, plans, dj, compress_on_device=True)
    assert sorted(os.listdir(out_a)) == sorted(os.listdir(out_b)) == sorted(n + '.nii.gz' for n in names)
    for n, p, src in zip(names, preds, files_pred):
        want = pp.apply_postprocessing(p, fns, kwargs)
        assert np.array_equal(want, ARRAYS[f'{name}__{n}__postprocessed'])
        values, info, blob = _file_labels(os.path.join(out_a, n + '.nii.gz'))
        assert np.array_equal(values, want) and int(info['header']['datatype']) == 2
        assert np.array_equal(info['affine'], nifti_ref.read(src)[1]['affine'])
        assert nifti_ref.file_bytes(os.path.join(out_b, n + '.nii.gz')) == blob
    single = os.path.join(tmp_path, 'single.nii.gz')
    from fast_nnunet_amd.imageio import NiftiIO
    pp.load_postprocess_save(files_pred[0], single, NiftiIO(), fns, kwargs)
    assert nifti_ref.file_bytes(single) == nifti_ref.file_bytes(os.path.join(out_a, names[0] + '.nii.gz'))


@pytest.mark.parametrize('name,dataset', [('labels_4_crop', 'labels3'), ('regions_3_crop', 'regions')])
def test_ensemble_folders_equals_the_array_functions(name, dataset, tmp_path):
    from fast_nnunet_amd import ensembling as ens
    from fast_nnunet_amd.plans import LabelManager
    from golden_cases import DATASET_JSONS
    z = np.load(os.path.join(GOLDEN, 'ensemble.npz'))
    members = [z[f'{name}__member{m}'] for m in range(3)]
    dj = dict(DATASET_JSONS[dataset], file_ending='.nii.gz')
    lm = LabelManager(dj['labels'], dj.get('regions_class_order'))
    props = {'nibabel_stuff': {'original_affine': AFFINE.copy()}, 'spacing': [0.5, 2.0, 1.5], 'shape_before_cropping': tuple(members[0].shape[1:])}
    cases = {'case_b': members, 'case_a': [m[:, ::-1].copy() for m in members]}
    folders = []
    for k in range(3):
        folders.append(os.path.join(tmp_path, f'member{k}'))
        os.makedirs(folders[-1])
        for case, ms in cases.items():
            np.savez_compressed(os.path.join(folders[-1], case + '.npz'), probabilities=ms[k])
            if k == 0:
                with open(os.path.join(folders[-1], case + '.pkl'), 'wb') as f:
                    pickle.dump(props, f)
    for n, obj in (('plans.json', PLANS), ('dataset.json', dj)):
        with open(os.path.join(folders[0], n), 'w') as f:
            json.dump(obj, f)
    out = os.path.join(tmp_path, 'merged')
    ens.ensemble_folders(folders, out, save_merged_probabilities=True)
    assert sorted(os.listdir(out)) == sorted(['dataset.json'] + [c + e for c in cases for e in ('.nii.gz', '.npz', '.pkl')])
    with open(os.path.join(out, 'dataset.json')) as f:
        assert json.load(f) == dj
    for case, ms in cases.items():
        want = ens.ensemble_probabilities(ms, lm)
        values, info, _ = _file_labels(os.path.join(out, case + '.nii.gz'))
        assert np.array_equal(values, want) and want.max() > 0
        assert np.array_equal(info['affine'], AFFINE)
        with np.load(os.path.join(out, case + '.npz'), allow_pickle=False) as f:
            avg = f['probabilities']
        assert avg.dtype == np.float32 and np.array_equal(avg.view(np.uint32), ens.average_probabilities(ms).view(np.uint32))
        got_props = ens.load_properties_pkl(os.path.join(out, case + '.pkl'))
        assert got_props.keys() == props.keys() and np.array_equal(got_props['nibabel_stuff']['original_affine'], AFFINE)
    if name == 'regions_3_crop':                                 # (the golden's map is that of exactly these three members)
        assert np.array_equal(_file_labels(os.path.join(out, 'case_b.nii.gz'))[0], z[f'{name}__seg'])
    # without the probabilities: the label files alone, and merge_files for one case
    out2 = os.path.join(tmp_path, 'merged_labels')
    ens.ensemble_folders(folders, out2, dataset_json_file_or_dict=dj, plans_json_file_or_dict=PLANS)
    assert sorted(os.listdir(out2)) == ['case_a.nii.gz', 'case_b.nii.gz', 'dataset.json']
    from fast_nnunet_amd.imageio import NiftiIO
    ens.merge_files([os.path.join(f, 'case_a.npz') for f in folders], os.path.join(tmp_path, 'one'), '.nii.gz', NiftiIO(), lm)
    assert nifti_ref.file_bytes(os.path.join(tmp_path, 'one.nii.gz')) == nifti_ref.file_bytes(os.path.join(out2, 'case_a.nii.gz')) \
        == nifti_ref.file_bytes(os.path.join(out, 'case_a.nii.gz'))
    assert not [t.name for t in threading.enumerate() if t.name.startswith('fnn-')]


@pytest.mark.parametrize('front_end', ['evaluate', 'postprocess'])
def test_a_truncated_third_file_raises_after_the_workers_have_ended(front_end, tmp_path):
    from fast_nnunet_amd import evaluation as ev
    from fast_nnunet_amd import postprocessing as pp
    from fast_nnunet_amd.imageio import NiftiIO
    names = [f'case_{i}' for i in range(4)]
    maps = [np.full((6, 7, 8), i + 1) for i in range(4)]
    _write_maps(os.path.join(tmp_path, 'ref'), names, maps, [(2, '<')])
    files = _write_maps(os.path.join(tmp_path, 'pred'), names, maps, [(4, '<')])
    blob = nifti_ref.file_bytes(files[2])
    with gzip.open(files[2], 'wb') as f:
        f.write(blob[:-100])
    out = os.path.join(tmp_path, 'out')
    with pytest.raises(RuntimeError, match='truncated') as e:
        if front_end == 'evaluate':
            ev.compute_metrics_on_folder(os.path.join(tmp_path, 'ref'), os.path.join(tmp_path, 'pred'),
                                         os.path.join(tmp_path, 'pred', 'summary.json'), NiftiIO(), '.nii.gz', [1, 2, 3, 4])
        else:
            pp.apply_postprocessing_to_folder(os.path.join(tmp_path, 'pred'), out,
                                              [pp.remove_all_but_largest_component_from_segmentation], [{'labels_or_regions': 1}],
                                              PLANS, {'labels': {'background': 0, 'a': 1}, 'file_ending': '.nii.gz'})
    assert files[2] in str(e.value)
    assert not [t.name for t in threading.enumerate() if t.name.startswith('fnn-')]
    left = [os.path.join(d, i) for d, _, fs in os.walk(tmp_path) for i in fs]
    assert not [i for i in left if '.part' in i] and not os.path.exists(os.path.join(tmp_path, 'pred', 'summary.json'))
    if front_end == 'postprocess':
        assert sorted(os.listdir(out)) == ['case_0.nii.gz', 'case_1.nii.gz']     # complete files only
