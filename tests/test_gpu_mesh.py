"""fnn_mesh_count / fnn_mesh_emit and fast_nnunet_amd.meshing on one MI355X against tests/mesh_ref.py: counts, boxes,
points, cells and the triangles' regions equal elementwise and in order, bit for bit, in both layouts.

The kernels' tiles: every kernel that walks a region's box owns 1024 raster-consecutive box corners (16 ballot words) or
1024 raster-consecutive box voxels per block; the only LDS is the 16 per-wave counts of a block (and 8 words per region
in the whole-map count).  There is no 3-D tile.  The shapes with one axis of 1030 put block boundaries inside lines, rows
and planes, (17, 33, 70) has 39 blocks per region, and the 64-corner word boundaries fall everywhere."""
import functools
import os

import numpy as np
import pytest
import torch

import mesh_ref as mr
from fast_nnunet_amd import capi, imageio, meshing

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'GenericAnatomyColors.txt')
GUARD, SENTINEL = 64, 0xA5
AFFINES = {'identity': np.eye(4).tolist(),
           'rotated': [[0.0, -0.7, 0.0, 12.5], [1.3, 0.0, 0.4, -3.0], [0.0, 0.2, 2.5, 40.0], [0, 0, 0, 1]],
           'flipped': [[-0.8, 0.1, 0.0, 90.0], [0.0, 0.9, 0.0, -20.0], [0.2, 0.0, 3.0, 5.0], [0, 0, 0, 1]]}
PAIRS = (0, 1, 7)
# what every scenario runs: the three affines, the three pair counts and the two layouts, each at least once
BASIC = [('identity', 0, 0), ('rotated', 1, 1), ('flipped', 7, 0)]
CROSS = [(a, p, l) for a in AFFINES for p in PAIRS for l in (0, 1)]


# ---- label maps: (seg, regions)
def dilate(m):
    out = m.copy()
    for ax in range(3):
        lo, hi = [slice(None)] * 3, [slice(None)] * 3
        lo[ax], hi[ax] = slice(0, -1), slice(1, None)
        out[tuple(hi)] |= m[tuple(lo)]
        out[tuple(lo)] |= m[tuple(hi)]
    return out


def s_random(shape, rng):
    return (rng.random(shape) < 0.4).astype(np.uint8), [[1]]


def s_full(shape, rng):                                              # one region that touches all six borders
    return np.ones(shape, np.uint8), [[1]]


def s_checker(shape, rng):
    return (np.indices(shape).sum(0) % 2).astype(np.uint8), [[1]]


def s_touching(shape, rng):
    seg = np.full(shape, 2, np.uint8)
    ax = int(np.argmax(shape))
    seg[tuple(slice(0, max(1, shape[ax] // 2)) if a == ax else slice(None) for a in range(3))] = 1
    return seg, [[1], [2]]


def s_two_label_region(shape, rng):
    return rng.integers(0, 4, shape).astype(np.uint8), [[1, 3], [2]]


def s_blobs16(shape, rng):                                           # uint16 labels above 255, separate blobs
    seg = np.zeros(shape, np.uint16)
    for label in (300, 1000, 65535):
        seg[dilate(dilate(rng.random(shape) < 25 / np.prod(shape)))] = label
    return seg, [[300], [1000], [65535]]


def s_absent_between(shape, rng):                                    # label 2 has no voxel: its empty block shifts nothing
    seg = rng.integers(0, 3, shape).astype(np.uint8)
    seg[seg == 2] = 3
    return seg, [[1], [2], [3]]


def s_overlapping(shape, rng):                                       # 3 regions that share labels and whose boxes overlap
    seg = rng.integers(0, 4, shape).astype(np.uint16)
    seg[seg == 3] = 700
    return seg, [[1, 2], [2, 700], [1, 700]]


def s_shell(shape, rng):                                             # both sides of a shell on the border, and a core
    seg = np.ones(shape, np.uint8)
    seg[tuple(slice(1, -1) for _ in shape)] = 0
    seg[tuple(n // 2 for n in shape)] = 2
    return seg, [[1], [2], [1, 2]]


SMALL = [(5, 7, 9), (1, 1, 1), (1, 6, 6), (4, 1, 1)]
LONG = [(1030, 3, 4), (3, 1030, 4), (3, 4, 1030)]
SCENARIOS = [(s, m, BASIC) for s in SMALL for m in (s_random, s_full, s_checker, s_touching, s_two_label_region)]
SCENARIOS += [((17, 33, 70), s_blobs16, CROSS), ((17, 33, 70), s_overlapping, BASIC), ((17, 33, 70), s_full, BASIC)]
SCENARIOS += [(s, m, BASIC) for s in LONG for m in (s_random, s_full)]
SCENARIOS += [((6, 9, 11), s_absent_between, BASIC), ((6, 9, 11), s_shell, BASIC), ((5, 7, 9), s_blobs16, BASIC)]
IDS = [f'{"x".join(map(str, s))}-{m.__name__[2:]}' for s, m, _ in SCENARIOS]


@functools.lru_cache(maxsize=None)
def scenario(k):
    shape, maker, _ = SCENARIOS[k]
    seg, regions = maker(shape, np.random.default_rng(1000 + k))
    seg.setflags(write=False)
    return seg, regions


@functools.lru_cache(maxsize=None)
def reference(k, affine, pairs):
    """mesh_ref's answer, computed once per (scenario, affine, pairs) and shared by the layouts and tests."""
    seg, regions = scenario(k)
    m = mr.mesh(seg, regions, affine=AFFINES[affine], pairs=pairs)
    for v in m.values():
        v.setflags(write=False)
    return m


def on_device(seg, offset=0):
    """The map on the GPU as the library takes it: uint8, or int16 with the bits of uint16; offset: elements into a larger
    tensor, so that the map is aligned to its element only."""
    arr = seg if seg.dtype == np.uint8 else seg.view(np.int16)
    big = torch.zeros(seg.size + offset + 3, dtype=torch.uint8 if seg.dtype == np.uint8 else torch.int16, device='cuda')
    view = big[offset:offset + seg.size]
    view.copy_(torch.from_numpy(arr.reshape(-1).copy()))
    assert offset == 0 or view.data_ptr() % 4 != 0
    return view


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


def emit(dev, seg, regions, affine, pairs, layout, cap_points=None, cap_cells=None, n=0, t=0):
    points, cells, region = Guarded(12 * n), Guarded((16 if layout else 12) * t), Guarded(2 * t)
    member = meshing._member_table(regions)
    capi.mesh_emit(dev.data_ptr(), seg.dtype == np.uint16, seg.shape, member, np.asarray(AFFINES[affine], np.float64), pairs, layout,
                   points.ptr, n if cap_points is None else cap_points, cells.ptr, t if cap_cells is None else cap_cells, region.ptr,
                   torch.cuda.current_stream().cuda_stream)
    return points, cells, region


def expected_bytes(ref, layout):
    if layout:
        return mr.vtk_payload(ref)
    return ref['points'].tobytes(), ref['triangles'].tobytes(), ref['triangle_region'].tobytes()


@pytest.mark.parametrize('k', range(len(SCENARIOS)), ids=IDS)
def test_counts_boxes_points_cells_and_regions_bit_for_bit(k):
    seg, regions = scenario(k)
    dev = on_device(seg)
    counts, boxes = capi.mesh_count(dev.data_ptr(), seg.dtype == np.uint16, seg.shape, meshing._member_table(regions),
                                    torch.cuda.current_stream().cuda_stream)
    ref0 = reference(k, 'identity', 0)
    assert np.array_equal(counts, ref0['counts']) and np.array_equal(boxes, ref0['boxes'])
    for affine, pairs, layout in SCENARIOS[k][2]:
        ref = reference(k, affine, pairs)
        n, t = len(ref['points']), len(ref['triangles'])
        got = emit(dev, seg, regions, affine, pairs, layout, n=n, t=t)
        for name, g, want in zip(('points', 'cells', 'cell_region'), got, expected_bytes(ref, layout)):
            assert g.guards_intact(), (name, affine, pairs, layout)
            have = g.bytes()
            if have != want:                                          # say where, then fail
                a, b = np.frombuffer(have, np.uint8), np.frombuffer(want, np.uint8)
                first = int(np.flatnonzero(a != b)[0])
                pytest.fail(f'{name} differ for {affine}, {pairs} pairs, layout {layout}: {int((a != b).sum())} of {len(a)} bytes, the first at {first}')


@pytest.mark.parametrize('offset', [1, 3])
@pytest.mark.parametrize('wide', [False, True], ids=['u8', 'u16'])
def test_a_map_that_is_a_slice_of_a_larger_tensor(offset, wide):
    k = next(i for i, (s, m, _) in enumerate(SCENARIOS) if s == (5, 7, 9) and m is (s_blobs16 if wide else s_two_label_region))
    seg, regions = scenario(k)
    dev = on_device(seg, offset)
    ref = reference(k, 'rotated', 1)
    counts, boxes = capi.mesh_count(dev.data_ptr(), wide, seg.shape, meshing._member_table(regions), torch.cuda.current_stream().cuda_stream)
    assert np.array_equal(counts, ref['counts']) and np.array_equal(boxes, ref['boxes'])
    got = emit(dev, seg, regions, 'rotated', 1, 1, n=len(ref['points']), t=len(ref['triangles']))
    assert [g.bytes() for g in got] == list(mr.vtk_payload(ref)) and all(g.guards_intact() for g in got)


@pytest.mark.parametrize('layout', [0, 1])
def test_a_cap_one_below_the_total_writes_nothing_and_says_so(layout):
    k = IDS.index('6x9x11-absent_between')
    seg, regions = scenario(k)
    dev = on_device(seg)
    ref = reference(k, 'identity', 0)
    n, t = len(ref['points']), len(ref['triangles'])
    lib = capi.load_library()
    for caps, text in (((n - 1, t), f'cap_points is below the number of points ({n})'), ((n, t - 1), f'cap_cells is below the number of triangles ({t})')):
        bufs = [Guarded(12 * n), Guarded(16 * t), Guarded(2 * t)]
        with pytest.raises(AssertionError) as e:
            capi.mesh_emit(dev.data_ptr(), False, seg.shape, meshing._member_table(regions), np.eye(4), 1, layout, bufs[0].ptr, caps[0],
                           bufs[1].ptr, caps[1], bufs[2].ptr, torch.cuda.current_stream().cuda_stream)
        assert str(e.value) == 'fnn_mesh_emit: ' + text and lib.fnn_last_error(None).decode() == str(e.value)
        torch.cuda.synchronize()
        assert all(b.untouched() for b in bufs)


def test_two_runs_give_equal_bytes():
    k = IDS.index('17x33x70-blobs16')
    seg, regions = scenario(k)
    dev = on_device(seg)
    ref = reference(k, 'rotated', 7)
    runs = [[g.bytes() for g in emit(dev, seg, regions, 'rotated', 7, 1, n=len(ref['points']), t=len(ref['triangles']))] for _ in range(2)]
    assert runs[0] == runs[1] == list(mr.vtk_payload(ref))


def test_an_empty_map_and_an_unreachable_label_launch_nothing_and_give_zeros():
    seg = np.zeros((4, 5, 6), np.uint8)
    dev = on_device(seg)
    stream = torch.cuda.current_stream().cuda_stream
    counts, boxes = capi.mesh_count(dev.data_ptr(), False, seg.shape, meshing._member_table([[1], [300]]), stream)
    assert not counts.any() and not boxes.any()
    bufs = [Guarded(16), Guarded(16), Guarded(16)]
    capi.mesh_emit(dev.data_ptr(), False, seg.shape, meshing._member_table([[1], [300]]), np.eye(4), 3, 1, bufs[0].ptr, 0, bufs[1].ptr, 0,
                   bufs[2].ptr, stream)
    torch.cuda.synchronize()
    assert all(b.untouched() for b in bufs)


def test_label_surfaces_takes_arrays_and_tensors_and_finds_the_labels():
    k = IDS.index('17x33x70-blobs16')
    seg, regions = scenario(k)
    ref = reference(k, 'rotated', 1)                                  # smoothing_factor 0.02 is one pair
    assert mr.smoothing_pairs(0.02) == 1
    on_gpu = torch.from_numpy(seg.view(np.int16).copy()).cuda()
    for given in (seg, seg.astype(np.int64), on_gpu, torch.from_numpy(seg.astype(np.int32))):
        m = meshing.label_surfaces(given, affine=AFFINES['rotated'], smoothing_factor=0.02)
        assert m.regions == [(300,), (1000,), (65535,)]
        assert np.array_equal(m.points.view(np.uint32), ref['points'].view(np.uint32)) and np.array_equal(m.triangles, ref['triangles'])
        assert np.array_equal(m.triangle_region, ref['triangle_region'])
        assert m.point_offsets.tolist() == [0] + np.cumsum(ref['counts'][:, 0]).tolist()
        assert m.triangle_offsets.tolist() == [0] + np.cumsum(2 * ref['counts'][:, 1]).tolist()
    # regions, spacing (z, y, x) and LPS
    m = meshing.label_surfaces(seg, [(300, 1000), 65535], spacing=(2.5, 0.75, 0.5), coordinate_system='LPS')
    want = mr.mesh(seg, [[300, 1000], [65535]], affine=np.diag([0.5, 0.75, 2.5, 1.0]), lps=True)
    assert np.array_equal(m.points.view(np.uint32), want['points'].view(np.uint32)) and np.array_equal(m.triangles, want['triangles'])
    empty = meshing.label_surfaces(np.zeros((3, 3, 3), np.uint8))
    assert empty.regions == [] and empty.points.shape == (0, 3) and empty.triangles.shape == (0, 3)


def test_a_label_file_becomes_a_coloured_model_file(tmp_path):
    rng = np.random.default_rng(5)
    seg = np.zeros((9, 12, 14), np.uint8)
    for label in (1, 2, 3):
        seg[dilate(rng.random(seg.shape) < 0.01)] = label
    assert set(np.unique(seg)) == {0, 1, 2, 3}
    affine = np.array([[-0.75, 0, 0, 100.0], [0, 0.75, 0.25, -50.0], [0, 0, 2.5, 12.5], [0, 0, 0, 1]])   # exact in the header's float32
    mask, out = str(tmp_path / 'mask.nii.gz'), str(tmp_path / 'model.vtk')
    imageio.write_label_file(seg, mask, affine)
    gen = meshing.VTKModelGenerator(color_file_path=GOLDEN)
    with pytest.raises(NotImplementedError, match='decimation_factor'):
        gen.generate_vtk_model(mask, out, decimation_factor=0.2)
    assert not os.path.exists(out)
    for system in ('RAS', 'LPS'):
        assert gen.generate_vtk_model(mask_path=mask, output_path=out, smoothing_factor=0.1, decimation_factor=0.0, coordinate_system=system) == out
        back = meshing.read_vtk_polydata(out)
        model = meshing.label_surfaces(seg, affine=affine, smoothing_factor=0.1, coordinate_system=system)
        want = mr.mesh(seg, [[1], [2], [3]], affine=affine, pairs=5, lps=system == 'LPS')
        assert model.regions == [(1,), (2,), (3,)]
        for have in (back['points'], model.points):
            assert np.array_equal(have.view(np.uint32), want['points'].view(np.uint32))
        assert np.array_equal(back['triangles'], want['triangles']) and np.array_equal(model.triangles, want['triangles'])
        assert np.array_equal(back['labels'], want['triangle_region'] + 1)
        table = meshing.read_color_table(GOLDEN)
        assert np.array_equal(back['colors'], np.array([table[i][1:] for i in (1, 2, 3)], np.uint8)[want['triangle_region']])
    # the same from a map that is still on the device, with the case's properties
    labels, properties = imageio.NiftiIO().read_label_map(mask)
    other = str(tmp_path / 'other.vtk')
    assert gen.generate_from_labels(labels, properties, other, smoothing_factor=0.1, coordinate_system='LPS') == other
    assert open(other, 'rb').read() == open(out, 'rb').read()
    assert sorted(os.listdir(tmp_path)) == ['mask.nii.gz', 'model.vtk', 'other.vtk']
