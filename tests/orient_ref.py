"""The numpy yardstick of the reorientation tests, written independently of fast_nnunet_amd/imageio.py.

An *orientation* is a (3, 2) array as nibabel states it: row i says which output (world, RAS+) axis the array's axis i runs
along and in which direction (+1 / -1), in nibabel's (x, y, z) index space.  The tests construct affines from an
orientation (``affine_of``), so the orientation an affine must give is known from its construction and never taken from
the code under test.  Arrays of the engine are (z, y, x): nibabel's index space reversed (``apply_zyx``).
"""
import itertools

import numpy as np

SIGNED_PERMUTATIONS = [(p, s) for p in itertools.permutations(range(3)) for s in itertools.product((1, -1), repeat=3)]
ROTATION_RAD = (0.2, -0.15, 0.1)
ZOOMS = (0.7, 1.3, 2.5)
EXTENTS = (5, 7, 9)


def ornt_of(perm, signs):
    return np.array([[perm[i], signs[i]] for i in range(3)], dtype=np.float64)


def rotation(rad=ROTATION_RAD):
    a, b, c = rad
    rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
    rz = np.array([[np.cos(c), -np.sin(c), 0], [np.sin(c), np.cos(c), 0], [0, 0, 1]])
    return rz @ ry @ rx


def affine_of(perm, signs, zooms=ZOOMS, origin=(-11.5, 20.25, 3.0), rot=None):
    """A voxel-to-world affine whose array axis i runs along world axis perm[i] in direction signs[i] with step zooms[i],
    the whole then turned by ``rot`` (a rotation well inside 45 degrees keeps the dominant axes)."""
    a = np.eye(4)
    m = np.zeros((3, 3))
    for i in range(3):
        m[perm[i], i] = signs[i] * zooms[i]
    a[:3, :3] = m if rot is None else rot @ m
    a[:3, 3] = origin
    return a


def index_map(ornt, shape_xyz):
    """M (4 x 4): the index into the original array of an index into the reoriented one, written down axis by axis: the
    original's axis i lies along the reoriented array's axis ornt[i, 0], counted backwards when ornt[i, 1] is -1."""
    m = np.zeros((4, 4))
    m[3, 3] = 1
    for i in range(3):
        o, d = int(ornt[i, 0]), ornt[i, 1]
        m[i, o] = d
        m[i, 3] = shape_xyz[i] - 1 if d < 0 else 0
    return m


def reoriented_affine(affine, ornt, shape_xyz):
    return np.asarray(affine, dtype=np.float64) @ index_map(ornt, shape_xyz)


def reoriented_shape(ornt, shape_xyz):
    out = [0, 0, 0]
    for i in range(3):
        out[int(ornt[i, 0])] = shape_xyz[i]
    return tuple(out)


def map_index(ornt, shape_xyz, idx):
    """The index in the reoriented array of index ``idx`` (x, y, z) of the original."""
    out = [0, 0, 0]
    for i in range(3):
        out[int(ornt[i, 0])] = shape_xyz[i] - 1 - idx[i] if ornt[i, 1] < 0 else idx[i]
    return tuple(out)


def apply_xyz(arr, ornt):
    """The array reoriented, in nibabel's index space, element by element semantics via flip and moveaxis."""
    out = arr
    for i in range(3):
        if ornt[i, 1] < 0:
            out = np.flip(out, i)
    return np.ascontiguousarray(np.moveaxis(out, [0, 1, 2], [int(ornt[i, 0]) for i in range(3)]))


def apply_zyx(arr, ornt):
    """The same for an engine array (z, y, x)."""
    return np.ascontiguousarray(apply_xyz(arr.transpose(2, 1, 0), ornt).transpose(2, 1, 0))


def invert(ornt):
    """The orientation that undoes ``ornt``: apply(apply(a, ornt), invert(ornt)) is a."""
    out = np.zeros((3, 2))
    for i in range(3):
        out[int(ornt[i, 0])] = [i, ornt[i, 1]]
    return out


def src_axis_flip(ornt):
    """(src_axis, flip) of fnn_reorient for engine arrays (z, y, x), found by reorienting an array of indices."""
    shape = (2, 3, 4)
    idx = np.stack(np.meshgrid(*[np.arange(s) for s in shape], indexing='ij'))            # idx[a][z, y, x] = index along a
    moved = [apply_zyx(idx[a], ornt) for a in range(3)]
    src, flip = [], []
    for d in range(3):
        step = [0, 0, 0]
        step[d] = 1
        for a in range(3):
            if moved[a].shape[d] > 1 and moved[a][tuple(step)] != moved[a][0, 0, 0]:
                src.append(a)
                flip.append(int(moved[a][0, 0, 0] != 0))
    assert sorted(src) == [0, 1, 2]
    return tuple(src), tuple(flip)


def numpy_reorient(a, src_axis, flip):
    """fnn_reorient's statement in numpy."""
    t = a.transpose(src_axis)
    axes = tuple(d for d in range(3) if flip[d])
    return np.ascontiguousarray(np.flip(t, axes) if axes else t)


def to_ras(values_zyx, affine):
    """A file's (z, y, x) array brought to the RAS frame by the orientation its affine was *read* to have here: the closest
    world axis of every column (enough for the tests' affines, which stay away from ties)."""
    ornt = closest_axes(affine)
    return apply_zyx(values_zyx, ornt), ornt


def closest_axes(affine):
    m = np.asarray(affine, dtype=np.float64)[:3, :3]
    m = m / np.sqrt((m * m).sum(0))
    out = np.zeros((3, 2))
    for i in range(3):
        o = int(np.argmax(np.abs(m[:, i])))
        out[i] = [o, np.sign(m[o, i])]
    assert sorted(out[:, 0]) == [0, 1, 2]
    return out
