"""Binary morphology on a real MI355X (fnn_binary_morphology, csrc/morph.hip; the word rule of csrc/morph_core.h): every device
result must equal the scipy restatement of tests/morph_ref.py exactly - all four operations, the three connectivities, 1, 2
and 5 iterations, both border values, both label dtypes and three densities on shapes chosen for the places the kernels can go
wrong (rows of two words and a tail, of exactly one word, of one voxel; extents of 1; a 2-D map; a set whose grown box is
clipped on three faces and is not the whole volume), the count the entry returns, empty and full sets, the return
conventions and the front ends.  No tolerance anywhere: the results are label maps."""
import gzip
import os
import pickle

import numpy as np
import pytest
import torch

import morph_ref as ref
import pp_morph_ref

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda', 0)
OPS = ['dilation', 'erosion', 'opening', 'closing']
SHAPES = {'two_words_and_a_tail': (5, 7, 130), 'one_word': (3, 4, 64), 'x1': (1, 9, 65), 'y1': (9, 1, 63), 'z1': (2, 3, 1),
          'several_blocks': (17, 19, 200), 'plane': (11, 70), 'corner_blob': (40, 40, 200)}
DENSITIES = (0.1, 0.5, 0.9)


def _pp():
    from fast_nnunet_amd import postprocessing as pp
    return pp


def _fn(op):
    return getattr(_pp(), f'binary_{op}_in_segmentation')


def _same(got, want, seg, what=''):
    assert got.dtype == seg.dtype and got.shape == seg.shape
    bad = np.argwhere(got != want)
    assert bad.size == 0, f'{what}: {len(bad)} voxels differ, first {bad[:5].tolist()}: got {got[tuple(bad[0])]}, want {want[tuple(bad[0])]}'


def _labels(u16):
    """(the set's two labels, another label, the fill label): above 255 for a uint16 map."""
    return ((300, 301), 700, 301) if u16 else ((1, 2), 3, 2)


def _random_map(key, density, u16, seed):
    """The mask of the set (a region of two labels) has the given density; a third label and background share the rest.  The
    corner blob: the set lives in a corner of the volume only, the third label everywhere."""
    shape = SHAPES[key]
    rng = np.random.default_rng(seed)
    (a, b), other, _ = _labels(u16)
    in_set = rng.random(shape) < density
    if key == 'corner_blob':
        keep = np.zeros(shape, bool)
        keep[0:6, 33:40, 189:200] = True
        in_set &= keep
    seg = np.where(rng.random(shape) < 0.3, other, 0)
    seg = np.where(in_set, np.where(rng.random(shape) < 0.5, a, b), seg)
    return seg.astype(np.uint16 if u16 else np.uint8)


@pytest.fixture(scope='module')
def maps():
    """Every random map of the file, made once and never written to."""
    out = {}
    for k, key in enumerate(SHAPES):
        for d, density in enumerate(DENSITIES):
            for u16 in (False, True):
                m = _random_map(key, density, u16, seed=1000 + 10 * k + d)
                m.setflags(write=False)
                out[key, density, u16] = m
    return out


@pytest.mark.parametrize('u16', [False, True], ids=['uint8', 'uint16'])
@pytest.mark.parametrize('op', OPS)
@pytest.mark.parametrize('key', list(SHAPES))
def test_device_equals_scipy_bit_for_bit(key, op, u16, maps):
    (a, b), _, fill = _labels(u16)
    fn, n_cases, n_changed = _fn(op), 0, 0
    for density in DENSITIES:
        seg = maps[key, density, u16]
        for connectivity in (6, 18, 26):
            for iterations in (1, 2, 5):
                for border_value in (0, 1):
                    kw = dict(labels_or_regions=[(a, b)], iterations=iterations, connectivity=connectivity, border_value=border_value)
                    if op in ref.ADDS:
                        kw['fill_label'] = fill
                    got = fn(seg, **kw)
                    want = ref.morph_ref(seg, op, **kw)
                    _same(got, want, seg, f'{op} {key} density {density} {kw}')
                    n_cases += 1
                    n_changed += int((want != seg).any())
    assert n_cases == 54 and n_changed > 0, 'no case of this shape changed a voxel: it shows nothing'


def test_corner_blob_box_is_clipped_on_three_faces_and_is_not_the_volume(maps):
    """What the shape is there for: the set's box touches the low x, high y and high z faces, and grown by 5 it is still a
    small part of the volume."""
    seg = maps['corner_blob', 0.5, False]
    idx = np.argwhere(np.isin(seg, (1, 2)))
    lo, hi = idx.min(0), idx.max(0)
    assert lo[0] == 0 and hi[1] == 39 and hi[2] == 199 and hi[0] + 5 < 39 and lo[1] - 5 > 0 and lo[2] - 5 > 0


def _entry(seg, table, op, connectivity, iterations, border_value, bg, fill, axes=7):
    """The C entry on a copy of ``seg`` (uint8 / uint16, 3-D): (result, changed)."""
    from fast_nnunet_amd import capi
    u16 = seg.dtype == np.uint16
    t = torch.from_numpy(seg.astype(np.int16) if u16 else seg.copy()).to(DEV)
    changed = capi.binary_morphology(t.data_ptr(), u16, t.shape, table, op, connectivity, iterations, border_value, bg, fill, axes)
    return t.cpu().numpy().view(seg.dtype), changed


def test_the_entry_returns_the_number_of_voxels_it_wrote(maps):
    from fast_nnunet_amd import capi
    for u16 in (False, True):
        (a, b), _, fill = _labels(u16)
        seg = maps['several_blocks', 0.5, u16]
        table = np.full(b + 1, -1, np.int32)
        table[[a, b]] = 0
        for code, op in enumerate(OPS):
            assert code == getattr(capi, {'dilation': 'FNN_MORPH_DILATE', 'erosion': 'FNN_MORPH_ERODE', 'opening': 'FNN_MORPH_OPEN',
                                          'closing': 'FNN_MORPH_CLOSE'}[op])
            for border_value in (0, 1):
                got, changed = _entry(seg, table, code, 26, 2, border_value, 0, fill)
                kw = dict(labels_or_regions=[(a, b)], iterations=2, connectivity=26, border_value=border_value)
                want = ref.morph_ref(seg, op, **kw, **({'fill_label': fill} if op in ref.ADDS else {}))
                _same(got, want, seg, f'{op} border {border_value}')
                assert changed == int((want != seg).sum())
        assert _entry(seg, table, capi.FNN_MORPH_ERODE, 6, 1, 0, 0, 0)[1] > 0
    # axes 7 on a (1, Y, Z) volume: the x-neighbours are outside the map and count as the border value, as scipy's for that array
    flat = maps['x1', 0.9, False]
    table = np.array([-1, 0, 0], np.int32)
    for border_value in (0, 1):
        got, _ = _entry(flat, table, capi.FNN_MORPH_ERODE, 6, 1, border_value, 0, 0, axes=7)
        _same(got, ref.morph_ref(flat, 'erosion', [(1, 2)], border_value=border_value), flat, f'(1, Y, Z) border {border_value}')
        got6, _ = _entry(flat, table, capi.FNN_MORPH_ERODE, 6, 1, border_value, 0, 0, axes=6)
        _same(got6[0], ref.morph_ref(flat[0], 'erosion', [(1, 2)], border_value=border_value), flat[0], f'plane border {border_value}')
    assert (_entry(flat, table, capi.FNN_MORPH_ERODE, 6, 1, 0, 0, 0, axes=7)[0] == 0).sum() > (flat == 0).sum()   # all of it goes: no x-neighbour


def test_hand_made_maps_on_the_device():
    for name, op, seg, kw, want in ref.cases():
        before = seg.copy()
        got = _fn(op)(seg, **kw)
        assert np.array_equal(seg, before), name
        _same(got, want, seg, name)


@pytest.mark.parametrize('shape', [(6, 7, 70), (9, 66)], ids=str)
def test_an_empty_set_and_a_set_that_fills_the_map(shape):
    pp = _pp()
    empty, full = np.full(shape, 4, np.uint8), np.full(shape, 1, np.uint8)
    for op in OPS:
        for border_value in (0, 1):
            for seg in (empty, full):
                kw = dict(labels_or_regions=[1], iterations=2, connectivity=18, border_value=border_value, background_label=4)
                _same(_fn(op)(seg, **kw), ref.morph_ref(seg, op, **kw), seg, f'{op} border {border_value} {"full" if seg is full else "empty"}')
    # what those are: with a zero border nothing grows out of an empty set and a full one is eroded from the faces; with a
    # border of 1 the empty map's outer layers fill and the full one stays
    assert np.array_equal(pp.binary_dilation_in_segmentation(empty, [1], border_value=0, background_label=4), empty)
    grown = pp.binary_dilation_in_segmentation(empty, [1], border_value=1, background_label=4)
    assert (grown == 1).sum() == empty.size - np.prod([s - 2 for s in shape])
    assert np.array_equal(pp.binary_erosion_in_segmentation(full, [1], border_value=1), full)
    assert (pp.binary_erosion_in_segmentation(full, [1], border_value=0) == 1).sum() == np.prod([s - 2 for s in shape])
    assert pp.binary_closing_in_segmentation(np.zeros((0, 4, 4), np.uint8), [1]).shape == (0, 4, 4)


def test_torch_in_torch_out_and_numpy_in_numpy_out(maps):
    pp = _pp()
    seg = maps['several_blocks', 0.5, False]
    kw = dict(labels_or_regions=[(1, 2)], iterations=2, connectivity=18)
    want = ref.morph_ref(seg, 'opening', **kw)
    got = pp.binary_opening_in_segmentation(seg, **kw)
    assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and np.array_equal(got, want)
    t = torch.from_numpy(seg.copy()).to(DEV)
    out = pp.binary_opening_in_segmentation(t, **kw)
    assert out.device == t.device and out.dtype == t.dtype and out.data_ptr() != t.data_ptr()
    assert np.array_equal(out.cpu().numpy(), want) and np.array_equal(t.cpu().numpy(), seg)
    host = torch.from_numpy(seg.copy())
    out = pp.binary_opening_in_segmentation(host, **kw)
    assert out.device.type == 'cpu' and np.array_equal(out.numpy(), want) and np.array_equal(host.numpy(), seg)
    for dtype in (np.int16, np.int32, np.int64, np.uint16):                      # wider integers come back as they came
        wide = maps['two_words_and_a_tail', 0.5, True].astype(dtype)
        kw16 = dict(labels_or_regions=[(300, 301)], fill_label=65535 if dtype != np.int16 else 32767, connectivity=26)
        got = pp.binary_closing_in_segmentation(wide, **kw16)
        assert got.dtype == dtype and np.array_equal(got, ref.morph_ref(wide, 'closing', **kw16))
    big = torch.from_numpy(maps['two_words_and_a_tail', 0.5, True].astype(np.int64)).to(DEV)
    out = pp.binary_dilation_in_segmentation(big, [300], iterations=3)
    assert out.dtype == torch.int64 and np.array_equal(out.cpu().numpy(), ref.morph_ref(big.cpu().numpy(), 'dilation', [300], iterations=3))
    again = pp.binary_dilation_in_segmentation(big, [300], iterations=3)
    assert torch.equal(out, again)                                               # two runs, the same bits


# ---- through the front ends ---------------------------------------------------------------------------------------------
def _organs():
    """Two organs with cavities, thin bridges and specks, and a third label inside one cavity."""
    rng = np.random.default_rng(34)
    seg = np.zeros((36, 40, 70), np.uint8)
    seg[4:16, 5:20, 6:30] = 1; seg[8:12, 9:15, 12:20] = 0; seg[10, 12, 15] = 3      # a hollow organ, a foreign label inside
    seg[9, 11, 30:40] = 1; seg[4:14, 5:15, 40:52] = 1                                # a bridge to a second blob of label 1
    seg[28:32, 4:8, 4:10] = 1                                                        # a third, small one, far from both
    seg[20:32, 22:36, 30:66] = 2; seg[25, 28, 44:47] = 0                            # organ 2 with a slit
    seg[rng.random(seg.shape) < 0.01] = 2                                            # specks of label 2 everywhere
    seg[6, 8, 8] = 0; seg[14, 18, 28] = 0                                            # pinholes in organ 1's wall
    return seg


def _chain(pp):
    fns = [pp.binary_closing_in_segmentation, pp.fill_holes_in_segmentation, pp.binary_opening_in_segmentation,
           pp.remove_all_but_largest_component_from_segmentation]
    kws = [{'labels_or_regions': 1}, {'labels_or_regions': 1}, {'labels_or_regions': 2, 'connectivity': 26, 'iterations': 2},
           {'labels_or_regions': [1]}]
    return fns, kws


def _chain_ref(seg, kws):
    seg = ref.morph_ref(seg, 'closing', **kws[0])
    seg = pp_morph_ref.apply_ref(seg, [('holes', kws[1])])
    seg = ref.morph_ref(seg, 'opening', **kws[2])
    return pp_morph_ref.apply_ref(seg, [('largest', kws[3])])


def test_apply_postprocessing_of_a_mixed_list_equals_the_model_with_one_upload_and_one_download(monkeypatch):
    pp = _pp()
    seg = _organs()
    fns, kws = _chain(pp)
    assert [k for k, _ in pp.plan_passes(fns, kws)] == ['gpu_morph', 'gpu_holes', 'gpu_morph', 'gpu']
    want = _chain_ref(seg, kws)
    steps = [ref.morph_ref(seg, 'closing', **kws[0])]
    steps.append(pp_morph_ref.apply_ref(steps[-1], [('holes', kws[1])]))
    steps.append(ref.morph_ref(steps[-1], 'opening', **kws[2]))
    assert (steps[0] != seg).any() and (steps[1] != steps[0]).any() and (steps[2] != steps[1]).any() and (want != steps[2]).any(), \
        'a step of the chain changes nothing: the case shows nothing'
    trips = []
    real = pp._postprocess
    monkeypatch.setattr(pp, '_postprocess', lambda s, passes: (trips.append(len(passes)), real(s, passes))[1])
    moves = {'up': 0, 'down': 0}                                                  # label maps that change sides during the call
    to, cpu = torch.Tensor.to, torch.Tensor.cpu

    def counted_to(self, *a, **k):
        out = to(self, *a, **k)
        if self.ndim >= 2 and out.device.type != self.device.type:
            moves['up' if out.device.type == 'cuda' else 'down'] += 1
        return out

    def counted_cpu(self, *a, **k):
        if self.ndim >= 2 and self.device.type == 'cuda':
            moves['down'] += 1
        return cpu(self, *a, **k)
    monkeypatch.setattr(torch.Tensor, 'to', counted_to)
    monkeypatch.setattr(torch.Tensor, 'cpu', counted_cpu)
    before = seg.copy()
    got = pp.apply_postprocessing(seg, fns, kws)
    monkeypatch.setattr(torch.Tensor, 'to', to)
    monkeypatch.setattr(torch.Tensor, 'cpu', cpu)
    assert trips == [4]                                                          # one trip to the device for the four passes
    assert moves == {'up': 1, 'down': 1}, moves                                  # and one map each way, none inside a pass
    assert np.array_equal(seg, before)
    _same(got, want, seg, 'chain')
    t = torch.from_numpy(seg).to(DEV)
    out = pp.apply_postprocessing(t, fns, kws)
    assert out.device == t.device and np.array_equal(out.cpu().numpy(), want) and np.array_equal(t.cpu().numpy(), seg)
    # the same list from a postprocessing.pkl
    fns2, kws2 = pp.load_postprocessing_pkl(pickle.dumps((fns, kws)))
    assert np.array_equal(pp.apply_postprocessing(seg, fns2, kws2), want)


def test_apply_postprocessing_to_folder_with_and_without_compression_on_the_device(tmp_path):
    from fast_nnunet_amd import imageio
    pp = _pp()
    affine = np.diag([1.5, 2.0, 0.5, 1.0])
    plans = {'dataset_name': 'd', 'plans_name': 'p', 'image_reader_writer': 'NibabelIO', 'configurations': {}}
    dataset = {'labels': {'background': 0, 'a': 1, 'b': 2, 'c': 3}, 'file_ending': '.nii.gz', 'channel_names': {'0': 'CT'}}
    src, want_dir = tmp_path / 'in', tmp_path / 'want'
    src.mkdir(); want_dir.mkdir()
    fns, kws = _chain(pp)
    segs = {'a': _organs(), 'b': np.ascontiguousarray(_organs()[::-1, :, ::-1])}
    for name, seg in segs.items():
        imageio.write_label_file(seg, str(src / f'{name}.nii.gz'), affine)
        imageio.write_label_file(_chain_ref(seg, kws), str(want_dir / f'{name}.nii.gz'), affine)
    outs = {}
    for flag in (False, True):
        outs[flag] = tmp_path / f'out_{int(flag)}'
        pp.apply_postprocessing_to_folder(str(src), str(outs[flag]), fns, kws, plans, dataset, compress_on_device=flag)
    for name in segs:
        made = [gzip.decompress((outs[flag] / f'{name}.nii.gz').read_bytes()) for flag in (False, True)]
        want = gzip.decompress((want_dir / f'{name}.nii.gz').read_bytes())
        assert made[0] == made[1] == want
        assert want != gzip.decompress((src / f'{name}.nii.gz').read_bytes())
    assert sorted(os.listdir(outs[True])) == ['a.nii.gz', 'b.nii.gz']
