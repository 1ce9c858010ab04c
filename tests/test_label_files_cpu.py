"""Label files without a GPU: ``read_label_map(on_device=False)`` against the restatement tests/label_files_ref.py on files
written by tests/nifti_ref.py, the refusals, the pairing rules and error texts of the folder front-ends (checked on empty or
tiny folders, before any GPU call is reached), and the restricted unpickler of the properties."""
import collections
import gzip
import json
import os
import pickle
import struct

import numpy as np
import pytest

import label_files_ref as lref
import nifti_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
SEG = 'example_ct_sm_T300_output.nii.gz'
CODES = sorted(lref.NIFTI_CODES)
SHAPE = (5, 6, 7)
# (name, slope, intercept, stored values): no scaling; an integral scaling; one that is integral only on even values
SCALINGS = {'none': (1.0, 0.0), 'integral': (2.0, 1.0), 'half': (0.5, 0.0)}


def _stored(code, scaling, wide):
    """Stored values every datatype holds (0..120) that are labels under ``scaling``; ``wide`` puts one label above 255 in."""
    n = int(np.prod(SHAPE))
    v = (np.arange(n) * 7 % 61) * 2                              # even, 0..120
    if wide:
        v[5] = {'none': 300, 'integral': 126, 'half': 126}[scaling] if lref.NIFTI_CODES[code] in ('u1', 'i1') else \
            {'none': 300, 'integral': 300, 'half': 2000}[scaling]
    return v.reshape(SHAPE)


def _expected(fname, itemsize):
    values, _ = nifti_ref.read(fname)
    out_bytes = 1 if itemsize == 1 else 2
    labels, flags, top = lref.file_labels(values, out_bytes)
    if out_bytes == 2 and top < 256:
        labels = labels.astype(np.uint8)
    return labels, flags


@pytest.mark.parametrize('order', ['<', '>'])
@pytest.mark.parametrize('code', CODES)
def test_host_route_equals_the_restatement(code, order, tmp_path):
    from fast_nnunet_amd.imageio import NiftiIO
    itemsize = np.dtype(lref.NIFTI_CODES[code]).itemsize
    seen = set()
    for scaling, (slope, inter) in SCALINGS.items():
        for wide in (False, True):
            if wide and itemsize == 1 and scaling == 'none':
                continue                                         # (a 1-byte file without scaling holds nothing above 255)
            fname = os.path.join(tmp_path, f'{scaling}_{int(wide)}.nii.gz')
            nifti_ref.write(fname, _stored(code, scaling, wide), code, order=order, slope=slope, inter=inter)
            want, flags = _expected(fname, itemsize)
            assert flags == 0
            got, props = NiftiIO().read_label_map(fname, on_device=False)
            assert isinstance(got, np.ndarray) and got.dtype == want.dtype and got.shape == SHAPE
            assert np.array_equal(got, want), (code, order, scaling, wide)
            assert props['spacing'] == [1.0, 1.0, 1.0] and 'nibabel_stuff' in props
            seen.add(got.dtype.name)
    assert seen == ({'uint8'} if itemsize == 1 else {'uint8', 'uint16'})


def test_half_slope_is_refused_on_an_odd_value(tmp_path):
    from fast_nnunet_amd.imageio import NiftiIO
    v = _stored(4, 'half', False)
    v[2, 3, 4] = 7
    fname = os.path.join(tmp_path, 'odd.nii')
    nifti_ref.write(fname, v, 4, slope=0.5)
    assert _expected(fname, 2)[1] == lref.NOT_INTEGRAL
    with pytest.raises(RuntimeError, match='not integral') as e:
        NiftiIO().read_label_map(fname, on_device=False)
    assert fname in str(e.value)


@pytest.mark.parametrize('case', ['fraction', 'nan', 'negative', 'above_uint8', 'above_uint16', 'two'])
def test_each_flag_raises_and_names_the_file(case, tmp_path):
    from fast_nnunet_amd.imageio import NiftiIO
    code, slope, value, flag, said = {
        'fraction': (16, 1.0, 1.5, lref.NOT_INTEGRAL, ['not integral']),
        'nan': (16, 1.0, np.nan, lref.NOT_INTEGRAL, ['not integral or not finite']),
        'negative': (4, 1.0, -1, lref.NEGATIVE, ['negative']),
        'above_uint8': (2, 2.0, 128, lref.TOO_LARGE, ['above 255']),
        'above_uint16': (8, 1.0, 65536, lref.TOO_LARGE, ['above 65535']),
        'two': (16, 1.0, -3.0, lref.NEGATIVE | lref.TOO_LARGE, ['negative', 'above 65535']),
    }[case]
    v = _stored(code, 'none', False).astype(lref.NIFTI_CODES[code]) // 2
    v[4, 5, 6] = value
    if case == 'two':
        v[0, 0, 0] = 70000.0
    fname = os.path.join(tmp_path, f'{case}.nii.gz')
    nifti_ref.write(fname, v, code, slope=slope)
    assert _expected(fname, v.dtype.itemsize)[1] == flag
    with pytest.raises(RuntimeError) as e:
        NiftiIO().read_label_map(fname, on_device=False)
    assert fname in str(e.value) and all(s in str(e.value) for s in said)
    for other in ('not integral', 'negative', 'above'):
        if not any(other in s for s in said):
            assert other not in str(e.value)


def test_the_reference_made_label_file_reads_as_its_bytes():
    from fast_nnunet_amd.imageio import NiftiIO, NiftiReorientIO
    fname = os.path.join(GOLDEN, SEG)
    with open(fname, 'rb') as f:
        blob = gzip.decompress(f.read())
    nx, ny, nz = struct.unpack_from('<3h', blob, 42)
    datatype, = struct.unpack_from('<h', blob, 70)
    off = int(struct.unpack_from('<f', blob, 108)[0])
    assert datatype == 2
    want = np.frombuffer(blob, np.uint8, nx * ny * nz, off).reshape(nz, ny, nx)
    got, props = NiftiIO().read_label_map(fname, on_device=False)
    assert got.dtype == np.uint8 and np.array_equal(got, want) and want.max() > 0
    ras, props_r = NiftiReorientIO().read_label_map(fname, on_device=False)
    images, props_i = NiftiReorientIO().read_images([fname], on_device=False)
    assert np.array_equal(ras, images[0].astype(np.uint8)) and props_r.keys() == props_i.keys()
    assert np.array_equal(props_r['nibabel_stuff']['reoriented_affine'], props_i['nibabel_stuff']['reoriented_affine'])


# ---------------------------------------------------------------------------------------------------------------
# the folder front-ends, up to where the GPU starts
# ---------------------------------------------------------------------------------------------------------------
PLANS = {'dataset_name': 'd', 'plans_name': 'p', 'image_reader_writer': 'NibabelIO', 'configurations': {}}
DATASET = {'labels': {'background': 0, 'a': 1}, 'file_ending': '.nii.gz', 'channel_names': {'0': 'CT'}}


def _folder(tmp_path, name, files=(), with_json=True):
    d = os.path.join(tmp_path, name)
    os.makedirs(d)
    for f in files:
        if f.endswith('.nii.gz'):
            nifti_ref.write(os.path.join(d, f), np.zeros((2, 2, 2)), 2)
        else:
            open(os.path.join(d, f), 'wb').close()
    if with_json:
        for n, obj in (('plans.json', PLANS), ('dataset.json', DATASET)):
            with open(os.path.join(d, n), 'w') as f:
                json.dump(obj, f)
    return d


def test_evaluation_pairing_rules(tmp_path):
    from fast_nnunet_amd import evaluation as ev
    from fast_nnunet_amd.imageio import NiftiIO
    ref = _folder(tmp_path, 'ref', ['a.nii.gz', 'b.nii.gz'], with_json=False)
    pred = _folder(tmp_path, 'pred', ['b.nii.gz', 'c.nii.gz', 'c.txt'], with_json=False)
    with pytest.raises(AssertionError, match='output_file should end with .json'):
        ev.compute_metrics_on_folder(ref, pred, os.path.join(pred, 'summary.txt'), NiftiIO(), '.nii.gz', [1])
    with pytest.raises(AssertionError, match='Not all files in folder_ref exist in folder_pred'):
        ev.compute_metrics_on_folder(ref, pred, None, NiftiIO(), '.nii.gz', [1], chill=False)
    # the cases are the sorted prediction files and the reference list is built from their names
    files_ref, files_pred = ev._paired_files(ref, pred, '.nii.gz', chill=True)
    assert files_pred == [os.path.join(pred, 'b.nii.gz'), os.path.join(pred, 'c.nii.gz')]
    assert files_ref == [os.path.join(ref, 'b.nii.gz'), os.path.join(ref, 'c.nii.gz')]
    empty = _folder(tmp_path, 'empty', with_json=False)
    with pytest.raises(ValueError, match='no case'):
        ev.compute_metrics_on_folder(ref, empty, None, NiftiIO(), '.nii.gz', [1])
    with pytest.raises(ValueError, match='ignore label'):
        ev.compute_metrics_on_folder(ref, empty, None, NiftiIO(), '.nii.gz', [1, 2], ignore_label=2)
    # the two wrappers default to <folder_pred>/summary.json: they get as far as the assertion with chill=False
    with pytest.raises(AssertionError, match='Not all files in folder_ref exist in folder_pred'):
        ev.compute_metrics_on_folder_simple(ref, pred, [1])
    plans, dataset = os.path.join(tmp_path, 'plans.json'), os.path.join(tmp_path, 'dataset.json')
    for n, obj in ((plans, PLANS), (dataset, DATASET)):
        with open(n, 'w') as f:
            json.dump(obj, f)
    with pytest.raises(AssertionError, match='Not all files in folder_ref exist in folder_pred'):
        ev.compute_metrics_on_folder2(ref, pred, dataset, plans)
    assert not os.path.exists(os.path.join(pred, 'summary.json'))


def test_postprocessing_folders_need_plans_and_dataset_json(tmp_path):
    from fast_nnunet_amd import postprocessing as pp
    bare = _folder(tmp_path, 'bare', with_json=False)
    out = os.path.join(tmp_path, 'out')
    with pytest.raises(RuntimeError, match='Expected plans file missing: .*plans.json. The plans file should have been'):
        pp.apply_postprocessing_to_folder(bare, out, [], [])
    with pytest.raises(RuntimeError, match='Expected plans file missing: .*dataset.json. The dataset.json should have been'):
        pp.apply_postprocessing_to_folder(bare, out, [], [], plans_file_or_dict=PLANS)
    with pytest.raises(RuntimeError, match='Expected plans file missing: .*plans.json. The plans files should have been'):
        pp.determine_postprocessing_on_folder(bare, bare)
    with pytest.raises(RuntimeError, match='Expected plans file missing: .*dataset.json. The plans files should have been'):
        pp.determine_postprocessing_on_folder(bare, bare, plans_file_or_dict=PLANS)
    assert not os.path.exists(out)
    # an empty folder with both files: nothing to do, and nothing but the folder is made
    full = _folder(tmp_path, 'full')
    pp.apply_postprocessing_to_folder(full, out, [], [])
    assert os.listdir(out) == []


def test_ensemble_folders_wants_the_same_members_everywhere(tmp_path):
    from fast_nnunet_amd import ensembling as ens
    a = _folder(tmp_path, 'a', ['x.npz', 'y.npz'])
    b = _folder(tmp_path, 'b', ['x.npz'])
    out = os.path.join(tmp_path, 'out')
    with pytest.raises(AssertionError, match='Not all folders contain the same files for ensembling. Please only '
                                             'provide folders that contain the predictions'):
        ens.ensemble_folders([a, b], out)
    assert not os.path.exists(out)
    # no member at all: dataset.json is copied and nothing else happens
    c, d = _folder(tmp_path, 'c'), _folder(tmp_path, 'd', with_json=False)
    ens.ensemble_folders([c, d], out)
    assert os.listdir(out) == ['dataset.json']
    with open(os.path.join(out, 'dataset.json')) as f:
        assert json.load(f) == DATASET


def test_determine_postprocessing_makes_an_output_folder_that_does_not_exist_yet(tmp_path):
    """The array function keeps its behaviour: ``output_folder`` (and ``postprocessed`` in it) is made by the call."""
    from evaluation_ref import HostBackend, dataset_maps, load_golden
    from fast_nnunet_amd import postprocessing as pp
    meta, arrays = load_golden()
    names, refs, preds = dataset_maps(meta, arrays, 'labels_fg_rejected')
    out = os.path.join(tmp_path, 'not', 'there', 'yet')
    fns, kwargs = pp.determine_postprocessing(dict(zip(names, preds)), dict(zip(names, refs)), meta['labels_fg_rejected']['dataset_json'],
                                              output_folder=out, backend=HostBackend())
    assert len(fns) == len(meta['labels_fg_rejected']['pp_fns']) == len(kwargs)
    assert sorted(os.listdir(out)) == ['postprocessed', 'postprocessing.json', 'postprocessing.pkl', 'summary.json']
    assert os.listdir(os.path.join(out, 'postprocessed')) == ['summary.json']


# ---------------------------------------------------------------------------------------------------------------
# the properties pickle
# ---------------------------------------------------------------------------------------------------------------
def _properties():
    affine = np.diag([1.5, 1.5, 2.0, 1.0])
    return {'nibabel_stuff': {'original_affine': affine, 'reoriented_affine': affine.copy()},
            'sitk_stuff': {'spacing': (1.5, 1.5, 2.0), 'origin': (0.0, -1.0, 2.0), 'direction': tuple(float(i) for i in np.eye(3).reshape(-1))},
            'spacing': [2.0, 1.5, 1.5], 'shape_before_cropping': (3, 4, 5), 'bbox_used_for_cropping': [[0, 3], [1, 4], [0, 5]],
            'shape_after_cropping_and_before_resampling': (3, 3, 5), 'a_numpy_scalar': np.float32(0.5), 'an_int': np.int64(7)}


def _same_properties(a, b):
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(_same_properties(a[k], b[k]) for k in a)
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and a.dtype == b.dtype and np.array_equal(a, b)
    if isinstance(a, (list, tuple)):
        return type(a) is type(b) and len(a) == len(b) and all(_same_properties(x, y) for x, y in zip(a, b))
    return type(a) is type(b) and a == b


def test_properties_unpickler_loads_what_the_predictor_exports(tmp_path):
    from fast_nnunet_amd import ensembling as ens
    from fast_nnunet_amd.case_pipeline import export_case_files
    props = _properties()
    probs = np.zeros((2, 3, 4, 5), np.float32)
    trunc = os.path.join(tmp_path, 'case')
    export_case_files(trunc, probs, props, lambda: None)         # (what the predictor's writer runs; no label file here)
    assert sorted(os.listdir(tmp_path)) == ['case.npz', 'case.pkl']
    got = ens.load_properties_pkl(trunc + '.pkl')
    assert _same_properties(got, props)
    with open(trunc + '.pkl', 'rb') as f:
        assert _same_properties(ens.load_properties_pkl(f.read()), props)


@pytest.mark.parametrize('what', ['function', 'class', 'object_array', 'reduce'])
def test_properties_unpickler_refuses_every_other_global(what):
    from fast_nnunet_amd import ensembling as ens

    class Reduce:
        def __reduce__(self):
            return os.getcwd, ()

    bad = {'function': {'spacing': os.getcwd}, 'class': collections.Counter(a=1),
           'object_array': np.array([{'a': 1}, None], dtype=object), 'reduce': Reduce()}[what]
    with pytest.raises(pickle.UnpicklingError, match='not allowed'):
        ens.load_properties_pkl(pickle.dumps({'x': bad}))


def test_symbol_and_abi():
    import re
    from fast_nnunet_amd import capi
    lib = capi.load_library()
    with open(os.path.join(os.path.dirname(GOLDEN), '..', 'include', 'fnn.h')) as f:
        header = f.read()
    assert re.search(r'\bfnn_decode_labels\s*\(', header) and 'fnn_decode_labels' in capi.EXPORTS and hasattr(lib, 'fnn_decode_labels')
    assert lib.fnn_abi_version() == 4 and re.search(r'#define\s+FNN_ABI_VERSION\s+4\b', header)
    assert (capi.LABEL_FLAG_NOT_INTEGRAL, capi.LABEL_FLAG_NEGATIVE, capi.LABEL_FLAG_TOO_LARGE) == \
        (lref.NOT_INTEGRAL, lref.NEGATIVE, lref.TOO_LARGE)
