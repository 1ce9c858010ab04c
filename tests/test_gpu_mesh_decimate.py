"""fnn_mesh_decimate and the decimation arguments of fast_nnunet_amd.meshing on one MI355X against
tests/mesh_decimate_ref.py: points, cells, triangle regions, per-region counts, rounds and exhausted equal elementwise and
in order, bit for bit, in both layouts, with the output buffers between sentinel guards.

The kernels' tiles: every kernel owns one vertex, triangle or half-edge per thread in blocks of 256, and the scans own 1024
values per block, so (17, 33, 70) `full` (16244 triangles, 48732 half-edges, 8124 points) crosses the block boundaries of
the lists, the scans and the compaction, and (1030, 2, 2) has 16496 triangles in one long strip.  The scenarios and their
parameters are tests/mesh_decimate_cases.py's."""
import os

import numpy as np
import pytest
import torch

import mesh_decimate_cases as mc
import mesh_decimate_ref as dr
import mesh_ref as mr
from fast_nnunet_amd import capi, imageio, meshing

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'GenericAnatomyColors.txt')
GUARD, SENTINEL = 64, 0xA5


class Guarded:
    """A device buffer of n bytes between two bands of sentinel bytes."""

    def __init__(self, n):
        self.n = n
        self.buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.uint8, device='cuda')
        self.ptr = self.buf.data_ptr() + GUARD

    def bytes(self):
        return self.buf[GUARD:GUARD + self.n].cpu().numpy().tobytes()

    def guards_intact(self):
        b = self.buf.cpu().numpy()
        return bool(np.all(b[:GUARD] == SENTINEL) and np.all(b[GUARD + self.n:] == SENTINEL))

    def untouched(self):
        return bool(np.all(self.buf.cpu().numpy() == SENTINEL))


def upload(arr):
    return torch.from_numpy(np.frombuffer(arr.tobytes() + b'\0' * 16, np.uint8).copy()).cuda()


def decimate(src, d, layout, n_out, t_out, cap_points=None, cap_cells=None):
    """One fnn_mesh_decimate call on a mesh_ref surface into guarded buffers of exactly the expected size."""
    dev = [upload(src[k]) for k in ('points', 'triangles', 'triangle_region')]
    out = [Guarded(12 * n_out), Guarded((16 if layout else 12) * t_out), Guarded(2 * t_out)]
    res = capi.mesh_decimate(dev[0].data_ptr(), len(src['points']), dev[1].data_ptr(), dev[2].data_ptr(), len(src['triangles']),
                             src['point_offsets'], d, layout, out[0].ptr, n_out if cap_points is None else cap_points, out[1].ptr,
                             t_out if cap_cells is None else cap_cells, out[2].ptr, torch.cuda.current_stream().cuda_stream)
    return out, res


def compare(got, want_bytes, what):
    for name, g, want in zip(('points', 'cells', 'cell_region'), got, want_bytes):
        assert g.guards_intact(), (name, what)
        have = g.bytes()
        if have != want:                                              # say where, then fail
            a, b = np.frombuffer(have, np.uint8), np.frombuffer(want, np.uint8)
            first = int(np.flatnonzero(a != b)[0])
            pytest.fail(f'{name} differ for {what}: {int((a != b).sum())} of {len(a)} bytes, the first at {first}')


@pytest.mark.parametrize('layout', [0, 1])
@pytest.mark.parametrize('k', range(len(mc.CASES)), ids=mc.IDS)
def test_points_cells_regions_counts_rounds_and_exhausted_bit_for_bit(k, layout):
    src, ref = mc.surface(k), mc.decimated(k)
    n_out, t_out = len(ref['points']), len(ref['triangles'])
    got, (counts, n, t, rounds, exhausted) = decimate(src, mc.CASES[k][4], layout, n_out, t_out)
    assert (n, t, rounds, exhausted) == (n_out, t_out, ref['rounds'], ref['exhausted'])
    assert np.array_equal(counts, ref['counts'])
    compare(got, dr.payload(ref, layout), f'{mc.IDS[k]}, layout {layout}')


def test_factor_zero_gives_the_bytes_of_the_emit():
    k = mc.IDS.index('9x12x14-blobs16-rotated-7-0.5')
    src = mc.surface(k)
    n, t = len(src['points']), len(src['triangles'])
    want_counts = np.stack([src['counts'][:, 0], 2 * src['counts'][:, 1]], 1)
    for layout, want in ((0, (src['points'].tobytes(), src['triangles'].tobytes(), src['triangle_region'].tobytes())), (1, mr.vtk_payload(src))):
        got, (counts, n_out, t_out, rounds, exhausted) = decimate(src, 0.0, layout, n, t)
        assert (n_out, t_out, rounds, exhausted) == (n, t, 0, 0) and np.array_equal(counts, want_counts)
        compare(got, want, f'factor 0, layout {layout}')


def test_two_runs_give_equal_bytes():
    k = mc.IDS.index('17x33x70-full-flipped-7-0.5')
    src, ref = mc.surface(k), mc.decimated(k)
    runs = [[g.bytes() for g in decimate(src, 0.5, 1, len(ref['points']), len(ref['triangles']))[0]] for _ in range(2)]
    assert runs[0] == runs[1] == list(dr.payload(ref, 1))


@pytest.mark.parametrize('layout', [0, 1])
def test_a_cap_one_below_the_result_writes_nothing_and_says_so(layout):
    k = mc.IDS.index('5x7x9-touching-flipped-0-0.5')
    src, ref = mc.surface(k), mc.decimated(k)
    n, t = len(ref['points']), len(ref['triangles'])
    lib = capi.load_library()
    for caps, text in (((n - 1, t), f'cap_points is below the number of points ({n})'), ((n, t - 1), f'cap_cells is below the number of triangles ({t})')):
        with pytest.raises(AssertionError) as e:
            got = [Guarded(12 * n), Guarded(16 * t), Guarded(2 * t)]
            dev = [upload(src[name]) for name in ('points', 'triangles', 'triangle_region')]
            capi.mesh_decimate(dev[0].data_ptr(), len(src['points']), dev[1].data_ptr(), dev[2].data_ptr(), len(src['triangles']),
                               src['point_offsets'], 0.5, layout, got[0].ptr, caps[0], got[1].ptr, caps[1], got[2].ptr,
                               torch.cuda.current_stream().cuda_stream)
        assert str(e.value) == 'fnn_mesh_decimate: ' + text and lib.fnn_last_error(None).decode() == str(e.value)
        torch.cuda.synchronize()
        assert all(g.untouched() for g in got)


def test_a_cell_outside_the_points_is_refused_and_nothing_is_written():
    k = mc.IDS.index('5x7x9-touching-flipped-0-0.5')
    src = dict(mc.surface(k))
    n, t = len(src['points']), len(src['triangles'])
    for bad in (n, -1):
        cells = src['triangles'].copy()
        cells[t // 2, 1] = bad
        with pytest.raises(AssertionError, match='names a point or a region that is not there'):
            got, _ = decimate(dict(src, triangles=cells), 0.5, 0, n, t)
    torch.cuda.synchronize()


def test_label_surfaces_decimates_like_decimate_surfaces_and_like_the_reference():
    k = mc.IDS.index('9x12x14-blobs16-rotated-7-0.5')
    seg, regions = mc.label_map(k)
    ref = mc.decimated(k)
    assert mr.smoothing_pairs(0.14) == 7
    kwargs = dict(labels_or_regions=regions, affine=mc.AFFINES['rotated'], smoothing_factor=0.14)
    direct = meshing.label_surfaces(seg, decimation_factor=0.5, **kwargs)
    plain = meshing.label_surfaces(seg, **kwargs)
    after = meshing.decimate_surfaces(plain, 0.5)
    assert (plain.rounds, plain.exhausted) == (0, 0) and len(plain.triangles) == len(mc.surface(k)['triangles'])
    for m in (direct, after):
        assert np.array_equal(m.points.view(np.uint32), ref['points'].view(np.uint32)) and np.array_equal(m.triangles, ref['triangles'])
        assert np.array_equal(m.triangle_region, ref['triangle_region'])
        assert (m.rounds, m.exhausted) == (ref['rounds'], ref['exhausted']) and m.regions == [tuple(r) for r in regions]
        assert m.point_offsets.tolist() == [0] + np.cumsum(ref['counts'][:, 0]).tolist()
        assert m.triangle_offsets.tolist() == [0] + np.cumsum(ref['counts'][:, 1]).tolist()
    same = meshing.decimate_surfaces(plain, 0.0)
    assert same.points.tobytes() == plain.points.tobytes() and same.triangles.tobytes() == plain.triangles.tobytes()
    empty = meshing.label_surfaces(np.zeros((3, 3, 3), np.uint8), decimation_factor=0.5)
    assert empty.regions == [] and empty.points.shape == (0, 3) and empty.triangles.shape == (0, 3)


def test_a_decimating_generator_writes_the_decimated_model(tmp_path):
    rng = np.random.default_rng(5)
    seg = np.zeros((9, 12, 14), np.uint8)
    for label in (1, 2, 3):
        seg[mc.dilate(mc.dilate(rng.random(seg.shape) < 0.004))] = label
    assert set(np.unique(seg)) == {0, 1, 2, 3}
    affine = np.array([[-0.75, 0, 0, 100.0], [0, 0.75, 0.25, -50.0], [0, 0, 2.5, 12.5], [0, 0, 0, 1]])   # exact in the header's float32
    mask, out = str(tmp_path / 'mask.nii.gz'), str(tmp_path / 'model.vtk')
    imageio.write_label_file(seg, mask, affine)
    gen = meshing.VTKModelGenerator(color_file_path=GOLDEN, decimation=True)
    table = meshing.read_color_table(GOLDEN)
    for system, d in (('RAS', 0.2), ('LPS', 0.5), ('RAS', 0.0)):                                          # 0.2: the reference's call
        assert gen.generate_vtk_model(mask_path=mask, output_path=out, smoothing_factor=0.1, decimation_factor=d, coordinate_system=system) == out
        back = meshing.read_vtk_polydata(out)
        surface = mr.mesh(seg, [[1], [2], [3]], affine=affine, pairs=5, lps=system == 'LPS')
        want = dr.decimate_mesh(surface, d)
        assert d == 0.0 or len(want['triangles']) < len(surface['triangles'])
        assert np.array_equal(back['points'].view(np.uint32), want['points'].view(np.uint32)) and np.array_equal(back['triangles'], want['triangles'])
        assert np.array_equal(back['labels'], np.repeat(np.array([1, 2, 3], np.uint16), want['counts'][:, 1]))
        assert np.array_equal(back['labels'], want['triangle_region'] + 1)
        assert np.array_equal(back['colors'], np.array([table[i][1:] for i in (1, 2, 3)], np.uint8)[want['triangle_region']])
    labels, properties = imageio.NiftiIO().read_label_map(mask)
    other = str(tmp_path / 'other.vtk')
    assert gen.generate_from_labels(labels, properties, other, smoothing_factor=0.1, decimation_factor=0.0) == other
    assert open(other, 'rb').read() == open(out, 'rb').read()
    assert sorted(os.listdir(tmp_path)) == ['mask.nii.gz', 'model.vtk', 'other.vtk']
