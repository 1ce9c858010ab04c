"""The scenarios the decimation tests share (tests/test_mesh_decimate_ref_cpu.py, tests/test_gpu_mesh_decimate.py): the
smallest shapes at which fnn_mesh_decimate's kernels can go wrong, each with one affine, smoothing pair count and factor, so
that the factors 0.2, 0.5, 0.9, the pair counts 0 and 7 and the three affines are each met several times without a full
cross.  The surface (tests/mesh_ref.py) and its decimation (tests/mesh_decimate_ref.py) are computed once per case."""
import functools

import numpy as np

import mesh_decimate_ref as dr
import mesh_ref as mr

AFFINES = {'identity': np.eye(4).tolist(),
           'rotated': [[0.0, -0.7, 0.0, 12.5], [1.3, 0.0, 0.4, -3.0], [0.0, 0.2, 2.5, 40.0], [0, 0, 0, 1]],
           'flipped': [[-0.8, 0.1, 0.0, 90.0], [0.0, 0.9, 0.0, -20.0], [0.2, 0.0, 3.0, 5.0], [0, 0, 0, 1]]}


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


def s_full(shape, rng):
    return np.ones(shape, np.uint8), [[1]]


def s_checker(shape, rng):
    return (np.indices(shape).sum(0) % 2).astype(np.uint8), [[1]]


def s_touching(shape, rng):
    seg = np.full(shape, 2, np.uint8)
    ax = int(np.argmax(shape))
    seg[tuple(slice(0, max(1, shape[ax] // 2)) if a == ax else slice(None) for a in range(3))] = 1
    return seg, [[1], [2]]


def s_blobs16(shape, rng):                                           # three uint16 blobs; region 400 between them has no voxel
    seg = np.zeros(shape, np.uint16)
    for label in (300, 1000, 65535):
        seg[dilate(dilate(rng.random(shape) < 25 / np.prod(shape)))] = label
    return seg, [[300], [400], [1000], [65535]]


def s_ellipsoid(shape, rng):                                         # semi-axes 0.42, 0.38, 0.45 of the shape about its centre
    g = np.indices(shape).astype(np.float64)
    r = sum(((g[k] - (shape[k] - 1) / 2) / (f * shape[k])) ** 2 for k, f in enumerate((0.42, 0.38, 0.45)))
    return (r <= 1.0).astype(np.uint8), [[1]]


def s_cuboid(shape, rng):                                            # 5x5x5 in 9^3
    seg = np.zeros(shape, np.uint8)
    seg[2:7, 2:7, 2:7] = 1
    return seg, [[1]]


#        shape         map          affine      pairs factor
CASES = [((1, 1, 1), s_full, 'identity', 0, 0.5),
         ((1, 1, 1), s_full, 'rotated', 7, 0.9),
         ((5, 7, 9), s_random, 'rotated', 7, 0.5),
         ((5, 7, 9), s_random, 'identity', 0, 0.9),
         ((5, 7, 9), s_checker, 'identity', 0, 0.9),
         ((5, 7, 9), s_touching, 'flipped', 0, 0.5),
         ((5, 7, 9), s_touching, 'rotated', 7, 0.9),
         ((9, 12, 14), s_blobs16, 'rotated', 7, 0.5),
         ((9, 12, 14), s_blobs16, 'flipped', 0, 0.2),
         ((17, 33, 70), s_full, 'identity', 0, 0.9),
         ((17, 33, 70), s_full, 'flipped', 7, 0.5),
         ((1030, 2, 2), s_full, 'flipped', 0, 0.2),
         ((14, 16, 18), s_ellipsoid, 'identity', 0, 0.2),
         ((14, 16, 18), s_ellipsoid, 'rotated', 7, 0.5),
         ((14, 16, 18), s_ellipsoid, 'identity', 0, 0.9),
         ((9, 9, 9), s_cuboid, 'identity', 0, 0.2),
         ((9, 9, 9), s_cuboid, 'identity', 0, 0.5),
         ((9, 9, 9), s_cuboid, 'identity', 0, 0.9)]
IDS = [f'{"x".join(map(str, s))}-{m.__name__[2:]}-{a}-{p}-{d}' for s, m, a, p, d in CASES]


@functools.lru_cache(maxsize=None)
def label_map(k):
    shape, maker = CASES[k][:2]
    seg, regions = maker(shape, np.random.default_rng(3000 + sum(shape)))
    seg.setflags(write=False)
    return seg, regions


@functools.lru_cache(maxsize=None)
def surface(k):
    """mesh_ref's surface of case k and its point offsets."""
    seg, regions = label_map(k)
    m = mr.mesh(seg, regions, affine=AFFINES[CASES[k][2]], pairs=CASES[k][3])
    m['point_offsets'] = np.concatenate([[0], np.cumsum(m['counts'][:, 0])]).astype(np.int64)
    for v in m.values():
        v.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def decimated(k):
    """mesh_decimate_ref's answer for case k."""
    out = dr.decimate_mesh(surface(k), CASES[k][4])
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out
