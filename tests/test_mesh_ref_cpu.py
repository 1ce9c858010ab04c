"""tests/mesh_ref.py, the yardstick of the surface kernels, pinned by invariants that do not come from it: face counts by
padding and comparing, the vertex and edge sets by looking at the voxels around every corner and edge, closedness, and the
enclosed volume, which fixes the winding table.  Then the colour table reader, the fallback colour and the VTK writer /
reader round trip, none of which needs a GPU."""
import itertools
import os

import numpy as np
import pytest

import mesh_ref as mr
from fast_nnunet_amd import meshing

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'GenericAnatomyColors.txt')
SHAPES = [(5, 7, 9), (1, 1, 1), (1, 6, 6), (4, 1, 1)]


def m_random(shape, rng):
    return (rng.random(shape) < 0.4).astype(np.uint8), [[1]]


def m_full(shape, rng):
    return np.ones(shape, np.uint8), [[1]]


def m_checker(shape, rng):
    return (np.indices(shape).sum(0) % 2).astype(np.uint8), [[1]]


def m_touching(shape, rng):
    seg = np.full(shape, 2, np.uint8)
    ax = int(np.argmax(shape))
    seg[tuple(slice(0, max(1, shape[ax] // 2)) if a == ax else slice(None) for a in range(3))] = 1
    return seg, [[1], [2]]


def m_two_label_region(shape, rng):
    return rng.integers(0, 4, shape).astype(np.uint8), [[1, 3], [2]]


MAPS = [m_random, m_full, m_checker, m_touching, m_two_label_region]
CASES = [(s, m) for s in SHAPES for m in MAPS]
IDS = [f'{"x".join(map(str, s))}-{m.__name__[2:]}' for s, m in CASES]


def make(shape, maker):
    return maker(shape, np.random.default_rng(sum(shape) * 7 + MAPS.index(maker)))


def padded(mask):
    p = np.zeros(tuple(n + 2 for n in mask.shape), bool)
    p[1:-1, 1:-1, 1:-1] = mask
    return p


def faces_by_padding(mask):
    p, n = padded(mask), 0
    for ax in range(3):
        for step in (-1, 1):
            n += int((p & ~np.roll(p, step, ax)).sum())              # the border of the padding is outside, so nothing wraps
    return n


def mixed_corners(mask):
    """{(cz, cy, cx)}: corners whose 8 surrounding voxels are neither all inside nor all outside, one corner at a time."""
    p, out = padded(mask), set()
    nz, ny, nx = mask.shape
    for cz, cy, cx in itertools.product(range(nz + 1), range(ny + 1), range(nx + 1)):
        around = p[cz:cz + 2, cy:cy + 2, cx:cx + 2]
        if around.any() and not around.all():
            out.add((cz, cy, cx))
    return out


def mixed_edges(mask):
    """{(corner, corner)}: lattice edges whose 4 surrounding voxels are neither all inside nor all outside."""
    p, out = padded(mask), set()
    nz, ny, nx = mask.shape
    for cz, cy, cx in itertools.product(range(nz + 1), range(ny + 1), range(nx + 1)):
        for ax in range(3):
            c = [cz, cy, cx]
            if c[ax] == mask.shape[ax]:
                continue
            sl = [slice(v, v + 2) for v in c]                        # padded voxels c-1 .. c around the corner
            sl[ax] = slice(c[ax] + 1, c[ax] + 2)                      # along the edge: the voxel layer the edge runs through
            around = p[tuple(sl)]
            if around.any() and not around.all():
                d = list(c)
                d[ax] += 1
                out.add((tuple(c), tuple(d)))
    return out


def region_parts(seg, values):
    mask = np.isin(seg, values)
    corners, tri, nbr, n_faces = mr.region_topology(mask)
    return mask, corners, tri, nbr, n_faces


@pytest.mark.parametrize('shape,maker', CASES, ids=IDS)
def test_faces_vertices_and_edges_are_what_the_voxels_say(shape, maker):
    seg, regions = make(shape, maker)
    for values in regions:
        mask, corners, tri, nbr, n_faces = region_parts(seg, values)
        assert n_faces == faces_by_padding(mask) and len(tri) == 2 * n_faces
        assert [tuple(c) for c in corners] == sorted(mixed_corners(mask))            # the set, in raster order
        assert np.array_equal(np.unique(tri), np.arange(len(corners)))              # exactly the corners the faces use
        want = mixed_edges(mask)
        smoothing = {(tuple(corners[i]), tuple(corners[j])) for i in range(len(corners)) for j in nbr[i] if j >= 0}
        assert smoothing == want | {(b, a) for a, b in want}
        assert np.all(((nbr >= 0).sum(1) >= 3) | (len(corners) == 0))
        for k, (dz, dy, dx) in enumerate(mr.NEIGHBOURS):                             # the order of the sum
            has = nbr[:, k] >= 0
            assert np.array_equal(corners[nbr[has, k]], corners[has] + (dz, dy, dx))
        ends = np.concatenate([tri[:, [0, 1]], tri[:, [1, 2]], tri[:, [2, 0]]])
        unit = np.abs(corners[ends[:, 0]] - corners[ends[:, 1]]).sum(1) == 1         # the quads' sides, not their diagonals
        of_faces = {tuple(sorted((tuple(corners[a]), tuple(corners[b])))) for a, b in ends[unit]}
        assert of_faces == want


@pytest.mark.parametrize('shape,maker', CASES, ids=IDS)
def test_every_edge_is_used_by_an_even_number_of_triangles(shape, maker):
    seg, regions = make(shape, maker)
    m = mr.mesh(seg, regions)
    t = m['triangles'].astype(np.int64)
    ends = np.sort(np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]]), 1)
    _, uses = np.unique(ends, axis=0, return_counts=True)
    assert np.all(uses % 2 == 0)


def six_volumes(points, triangles):
    p = points.astype(np.float64)
    a, b, c = p[triangles[:, 0]], p[triangles[:, 1]], p[triangles[:, 2]]
    return float((a * np.cross(b, c)).sum())


AFFINES = {'rotated': [[0.0, -0.7, 0.0, 12.5], [1.3, 0.0, 0.4, -3.0], [0.0, 0.2, 2.5, 40.0], [0, 0, 0, 1]],
           'flipped': [[-0.8, 0.1, 0.0, 90.0], [0.0, 0.9, 0.0, -20.0], [0.2, 0.0, 3.0, 5.0], [0, 0, 0, 1]]}


@pytest.mark.parametrize('shape,maker', CASES, ids=IDS)
def test_the_enclosed_volume_is_the_voxel_count(shape, maker):
    seg, regions = make(shape, maker)
    for r, values in enumerate(regions):
        n_vox = int(np.isin(seg, values).sum())
        m = mr.mesh(seg, [values])
        assert six_volumes(m['points'], m['triangles']) == 6 * n_vox                 # integers and halves in float64: exact
        for name, affine in AFFINES.items():
            w = mr.mesh(seg, [values], affine=affine)
            det = np.linalg.det(np.asarray(affine, np.float64)[:3, :3])
            assert (det < 0) == (name == 'flipped')
            # every coordinate is off by at most 2^-24 of its size M: a term a . (b x c) has 6 products of three coordinates,
            # each off by at most 3 * 2^-24 * M^3 to first order
            big = float(np.abs(w['points']).max()) if len(w['points']) else 0.0
            bound = len(w['triangles']) * 18 * 2.0 ** -24 * big ** 3 * 1.01
            assert abs(six_volumes(w['points'], w['triangles']) - 6 * n_vox * abs(det)) <= bound
            lps = mr.mesh(seg, [values], affine=affine, lps=True)
            assert np.array_equal(lps['triangles'], w['triangles'])
            assert np.array_equal(lps['points'], w['points'] * np.float32([-1, -1, 1]))


def test_smoothing_keeps_the_volume_of_a_ball_and_the_topology():
    z, y, x = np.indices((21, 21, 21)) - 10
    seg = (z * z + y * y + x * x <= 81).astype(np.uint8)
    n_vox = int(seg.sum())
    assert n_vox == 3071
    raw, smooth = mr.mesh(seg, [[1]]), mr.mesh(seg, [[1]], pairs=10)
    assert np.array_equal(raw['triangles'], smooth['triangles']) and raw['points'].shape == smooth['points'].shape
    assert np.array_equal(raw['counts'], smooth['counts'])
    assert abs(six_volumes(smooth['points'], smooth['triangles']) / 6 - n_vox) <= 0.01 * n_vox
    assert not np.array_equal(raw['points'], smooth['points'])
    assert smooth['points'].dtype == np.float32 and smooth['index_points'].dtype == np.float32


def test_regions_are_concatenated_and_an_absent_one_is_empty():
    seg = np.zeros((4, 5, 6), np.uint8)
    seg[1:3, 1:4, 1:3] = 1
    seg[0:2, 2:5, 3:6] = 3
    m = mr.mesh(seg, [[1], [2], [3]])
    assert m['counts'].tolist() == [[34, 32], [0, 0], [44, 42]]
    assert m['boxes'].tolist() == [[1, 3, 1, 4, 1, 3], [0] * 6, [0, 2, 2, 5, 3, 6]]
    assert m['triangle_region'].tolist() == [0] * 64 + [2] * 84
    assert m['triangles'][:64].max() == 33 and m['triangles'][64:].min() == 34 and m['triangles'].max() == 77
    assert mr.smoothing_pairs(0.5) == 25 and mr.smoothing_pairs(0.0) == 0 and mr.smoothing_pairs(1.0) == 50


# ---- colours and the file
def test_the_golden_colour_table_reads():
    table = meshing.read_color_table(GOLDEN)
    assert table[0] == ('background', 0, 0, 0, 0)
    assert table[1] == ('tissue', 128, 174, 128, 255) and table[2] == ('bone', 241, 214, 145, 255) and table[3] == ('skin', 177, 122, 101, 255)
    assert len(table) > 100 and all(len(v) == 5 for v in table.values())
    colors = meshing.region_colors([(3,), (2, 1), (60000,)], table)
    assert colors.tolist() == [[177, 122, 101, 255], [128, 174, 128, 255], list(mr.fallback_color(60000)[1:])]


def test_a_malformed_colour_line_names_the_file_and_the_line(tmp_path):
    path = tmp_path / 'colors.txt'
    for bad in ('4 name 1 2 3', '4 name 1 2 3 x', '4 name 1 2 3 256', '-1 name 1 2 3 4'):
        path.write_text('# comment\n1 a 1 2 3 4   # fine\n\n' + bad + '\n')
        with pytest.raises(ValueError, match=r'colors\.txt:4: '):
            meshing.read_color_table(str(path))
    path.write_text('# only a comment\n 7 x 1 2 3 4 # seven\n')
    assert meshing.read_color_table(str(path)) == {7: ('x', 1, 2, 3, 4)}


def test_the_fallback_colour_rule():
    assert meshing.fallback_color(0) == ('label_0', 255, 0, 0, 255)
    for lid in (1, 2, 7, 255, 4096, 65535):
        assert meshing.fallback_color(lid) == mr.fallback_color(lid)
        name, r, g, b, a = meshing.fallback_color(lid)
        assert name == f'label_{lid}' and a == 255 and max(r, g, b) == 255 and min(r, g, b) == 0     # full saturation and value
    assert len({meshing.fallback_color(k)[1:] for k in range(1, 62)}) == 61
    assert meshing.region_colors([(5,), (9, 4)]).tolist() == [list(mr.fallback_color(5)[1:]), list(mr.fallback_color(4)[1:])]


def model_of(seg, regions, **kw):
    m = mr.mesh(seg, regions, **kw)
    return meshing.SurfaceModel(m['points'], m['triangles'], m['triangle_region'], [tuple(r) for r in regions],
                                np.concatenate([[0], np.cumsum(m['counts'][:, 0])]), np.concatenate([[0], 2 * np.cumsum(m['counts'][:, 1])]))


def test_the_file_round_trip_is_exact(tmp_path):
    seg, regions = make((5, 7, 9), m_two_label_region)
    model = model_of(seg, regions, affine=AFFINES['rotated'], pairs=2)
    n, t = len(model.points), len(model.triangles)
    path = str(tmp_path / 'model.vtk')
    table = meshing.read_color_table(GOLDEN)
    meshing.write_vtk_polydata(model, path, table)
    assert os.listdir(tmp_path) == ['model.vtk']                                    # no part file is left
    blob = open(path, 'rb').read()
    head = f'# vtk DataFile Version 3.0\n{meshing.VTK_TITLE}\nBINARY\nDATASET POLYDATA\nPOINTS {n} float\n'.encode()
    assert blob.startswith(head)
    at = len(head)
    assert blob[at:at + 12 * n] == model.points.astype('>f4').tobytes()
    at += 12 * n
    polys = f'\nPOLYGONS {t} {4 * t}\n'.encode()
    assert blob[at:at + len(polys)] == polys
    at += len(polys)
    assert blob[at:at + 16 * t] == mr.vtk_payload({'points': model.points, 'triangles': model.triangles, 'triangle_region': model.triangle_region})[1]
    at += 16 * t
    cell = f'\nCELL_DATA {t}\nSCALARS label unsigned_short 1\nLOOKUP_TABLE default\n'.encode()
    assert blob[at:at + len(cell)] == cell
    at += len(cell) + 2 * t
    color = b'\nCOLOR_SCALARS colors 4\n'
    assert blob[at:at + len(color)] == color
    assert len(blob) == at + len(color) + 4 * t + 1 and blob.endswith(b'\n')
    back = meshing.read_vtk_polydata(path)
    assert back['title'] == meshing.VTK_TITLE
    assert back['points'].dtype == np.float32 and np.array_equal(back['points'].view(np.uint32), model.points.view(np.uint32))
    assert back['triangles'].dtype == np.int32 and np.array_equal(back['triangles'], model.triangles)
    ids = np.array([1, 2], np.uint16)[model.triangle_region]                         # the smallest id of (1, 3) and of (2,)
    assert np.array_equal(back['labels'], ids)
    assert np.array_equal(back['colors'], np.array([table[1][1:], table[2][1:]], np.uint8)[model.triangle_region])
    # explicit colours, no colours, an empty model
    meshing.write_vtk_polydata(model, path, np.array([[1, 2, 3, 4], [5, 6, 7, 8]], np.uint8))
    assert np.array_equal(meshing.read_vtk_polydata(path)['colors'], np.array([[1, 2, 3, 4], [5, 6, 7, 8]], np.uint8)[model.triangle_region])
    meshing.write_vtk_polydata(model, path)
    assert meshing.read_vtk_polydata(path)['colors'][0].tolist() == list(mr.fallback_color(1)[1:])
    empty = model_of(np.zeros((2, 2, 2), np.uint8), [[1]])
    meshing.write_vtk_polydata(empty, path)
    back = meshing.read_vtk_polydata(path)
    assert back['points'].shape == (0, 3) and back['triangles'].shape == (0, 3) and len(back['labels']) == 0
    with open(path, 'ab') as f:
        f.write(b'x')
    with pytest.raises(ValueError, match='after the last section'):
        meshing.read_vtk_polydata(path)
