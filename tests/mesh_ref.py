"""The surface of a label map as fnn_mesh_count / fnn_mesh_emit (csrc/mesh.hip) must give it, restated in numpy: the faces
between a region and everything else, their corners as vertices, the winding, Taubin smoothing in float32 and the float64
world transform.  tests/test_mesh_ref_cpu.py pins this file by invariants that do not come from it; the GPU tests compare
the library with it bit for bit.

Axes: the map is seg[z][y][x].  Corner (cz, cy, cx) of the (nz+1)(ny+1)(nx+1) corner grid has the index-space position
(x, y, z) = (cx - 0.5, cy - 0.5, cz - 0.5); voxel (z, y, x) lies between the corners (z, y, x) and (z+1, y+1, x+1)."""
import colorsys

import numpy as np

# face directions in their order inside one voxel, as (dz, dy, dx)
DIRS = ((-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1))
# the four corners of the face in direction k as (dz, dy, dx) from the voxel's lowest corner, in raster order q0 < q1 < q2 < q3
FACE_CORNERS = (((0, 0, 0), (0, 0, 1), (0, 1, 0), (0, 1, 1)),      # -z
                ((1, 0, 0), (1, 0, 1), (1, 1, 0), (1, 1, 1)),      # +z
                ((0, 0, 0), (0, 0, 1), (1, 0, 0), (1, 0, 1)),      # -y
                ((0, 1, 0), (0, 1, 1), (1, 1, 0), (1, 1, 1)),      # +y
                ((0, 0, 0), (0, 1, 0), (1, 0, 0), (1, 1, 0)),      # -x
                ((0, 0, 1), (0, 1, 1), (1, 0, 1), (1, 1, 1)))      # +x
# the two triangles of the face in direction k as indices into q0..q3: the quad is split along q0 - q3, and (b - a) x (c - a)
# points out of the region when (x, y, z) is a right-handed triple
_OUT, _IN = ((0, 1, 3), (0, 3, 2)), ((0, 3, 1), (0, 2, 3))
TRIANGLES = (_IN, _OUT, _OUT, _IN, _IN, _OUT)
# smoothing: neighbour directions in the order of the sum, as (dz, dy, dx), and the octant bits (bit dz*4 + dy*2 + dx of the 8
# voxels around a corner, d = 0 the lower one) of the 4 voxels around the lattice edge in that direction
NEIGHBOURS = ((0, 0, -1), (0, 0, 1), (0, -1, 0), (0, 1, 0), (-1, 0, 0), (1, 0, 0))
EDGE_OCTANTS = (0x55, 0xAA, 0x33, 0xCC, 0x0F, 0xF0)
RCP = np.array([0.0] + [1.0 / n for n in range(1, 7)]).astype(np.float32)
SMOOTH_F = (np.float32(0.5), np.float32(-0.53))                     # one pair: a pass with each factor
PAIRS_AT_FACTOR_ONE = 50                                            # smoothing_factor s -> round(50 s) pairs
GOLDEN = 0.6180339887498949


def smoothing_pairs(smoothing_factor):
    return int(round(PAIRS_AT_FACTOR_ONE * float(smoothing_factor)))


def fallback_color(label_id):
    """The colour of an id without a table entry: hue frac(id * 0.6180339887498949) at full saturation and value,
    every channel round(255 c), alpha 255."""
    r, g, b = colorsys.hsv_to_rgb((int(label_id) * GOLDEN) % 1.0, 1.0, 1.0)
    return (f'label_{int(label_id)}', int(round(255 * r)), int(round(255 * g)), int(round(255 * b)), 255)


def octants(mask):
    """uint8 [nz+1][ny+1][nx+1]: bit dz*4 + dy*2 + dx - voxel (cz-1+dz, cy-1+dy, cx-1+dx) is in the mask."""
    nz, ny, nx = mask.shape
    p = np.zeros((nz + 2, ny + 2, nx + 2), bool)
    p[1:-1, 1:-1, 1:-1] = mask
    o = np.zeros((nz + 1, ny + 1, nx + 1), np.uint8)
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                o |= p[dz:dz + nz + 1, dy:dy + ny + 1, dx:dx + nx + 1].astype(np.uint8) << (dz * 4 + dy * 2 + dx)
    return o


def region_topology(mask):
    """One region's (corners [n][3] int64 as (cz, cy, cx) in raster order, triangles int64 [2 faces][3] of indices into them
    for a positive determinant, neighbours int64 [n][6] with -1 for none, n_faces)."""
    nz, ny, nx = mask.shape
    p = np.zeros((nz + 2, ny + 2, nx + 2), bool)
    p[1:-1, 1:-1, 1:-1] = mask
    face = np.zeros((nz, ny, nx, 6), bool)
    for k, (dz, dy, dx) in enumerate(DIRS):
        face[..., k] = mask & ~p[1 + dz:1 + dz + nz, 1 + dy:1 + dy + ny, 1 + dx:1 + dx + nx]
    o = octants(mask)
    mixed = (o != 0) & (o != 255)
    vid = np.cumsum(mixed.ravel()).reshape(mixed.shape) - 1
    corners = np.argwhere(mixed)
    fz, fy, fx, fk = np.nonzero(face)                               # raster order of the voxel, then the direction
    fc = np.asarray(FACE_CORNERS)[fk]                               # [faces][4][3]
    q = vid[fz[:, None] + fc[..., 0], fy[:, None] + fc[..., 1], fx[:, None] + fc[..., 2]]
    order = np.asarray(TRIANGLES)[fk]                               # [faces][2][3]
    tri = np.take_along_axis(q[:, None, :].repeat(2, 1), order, 2).reshape(-1, 3)
    nbr = np.full((len(corners), 6), -1, np.int64)
    oc = o[mixed]
    for k, ((dz, dy, dx), m) in enumerate(zip(NEIGHBOURS, EDGE_OCTANTS)):
        part = oc & m
        has = (part != 0) & (part != m)
        c = corners[has] + (dz, dy, dx)
        nbr[has, k] = vid[c[:, 0], c[:, 1], c[:, 2]]
    return corners, tri, nbr, len(fz)


def smooth(pos, nbr, pairs):
    """pairs x (a Jacobi pass with f = 0.5, one with f = -0.53) on float32 positions [n][3]; every operation rounds."""
    pos = pos.astype(np.float32)
    present = nbr >= 0
    rcp = RCP[present.sum(1)][:, None]
    for _ in range(pairs):
        for f in SMOOTH_F:
            s = np.zeros_like(pos)
            for k in range(6):
                s = s + np.where(present[:, k, None], pos[nbr[:, k]], np.float32(0))
            m = s * rcp
            pos = pos + f * (m - pos)
    return pos


def to_world(pos, affine):
    """float32 index-space (x, y, z) [n][3] -> float32 world: ((A[r][0] x + A[r][1] y) + A[r][2] z) + A[r][3] in float64."""
    a = np.asarray(affine, np.float64)
    x, y, z = (pos[:, k].astype(np.float64) for k in range(3))
    out = np.empty((len(pos), 3), np.float32)
    for r in range(3):
        out[:, r] = (((a[r, 0] * x + a[r, 1] * y) + a[r, 2] * z) + a[r, 3]).astype(np.float32)
    return out


def mesh(seg, regions, affine=None, pairs=0, lps=False):
    """What the two entry points give for ``regions`` (a list of label-value lists): a dict with counts int64 [R][2]
    (vertices, faces), boxes int64 [R][6] (lo_z, hi_z, lo_y, hi_y, lo_x, hi_x), points float32 [n][3], triangles int32 [m][3],
    triangle_region uint16 [m], and the index-space positions after smoothing (``index_points``)."""
    a = np.eye(4) if affine is None else np.array(affine, np.float64)
    if lps:
        a[:2] = -a[:2]
    flip = np.linalg.det(a[:3, :3]) < 0
    counts, boxes = np.zeros((len(regions), 2), np.int64), np.zeros((len(regions), 6), np.int64)
    pts, ipts, tris, reg, base = [], [], [], [], 0
    for r, values in enumerate(regions):
        mask = np.isin(seg, list(values))
        if not mask.any():
            continue
        w = np.argwhere(mask)
        boxes[r] = np.stack([w.min(0), w.max(0) + 1], 1).ravel()
        corners, tri, nbr, n_faces = region_topology(mask)
        counts[r] = (len(corners), n_faces)
        pos = (corners[:, ::-1].astype(np.float32) - np.float32(0.5))
        pos = smooth(pos, nbr, pairs)
        if flip:
            tri = tri[:, [0, 2, 1]]
        ipts.append(pos)
        pts.append(to_world(pos, a))
        tris.append(tri + base)
        reg.append(np.full(len(tri), r, np.uint16))
        base += len(corners)
    cat = lambda parts, shape, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(shape, dt)
    return {'counts': counts, 'boxes': boxes, 'points': cat(pts, (0, 3), np.float32), 'triangles': cat(tris, (0, 3), np.int32),
            'triangle_region': cat(reg, (0,), np.uint16), 'index_points': cat(ipts, (0, 3), np.float32)}


def vtk_payload(m):
    """The layout-1 bytes of a mesh(): big-endian points, [3, a, b, c] big-endian cells, big-endian regions."""
    cells = np.concatenate([np.full((len(m['triangles']), 1), 3, np.int32), m['triangles']], 1)
    return m['points'].astype('>f4').tobytes(), cells.astype('>i4').tobytes(), m['triangle_region'].astype('>u2').tobytes()
