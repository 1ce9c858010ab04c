"""The rule of the small-component and hole-filling steps restated with scipy and numpy: what tests/test_pp_morph_cpu.py
checks on hand-made maps and tests/test_gpu_pp_morph.py compares the device results with, bit for bit.

* small components: ``ndimage.label`` of the mask ``seg in S`` with ``generate_binary_structure(ndim, ndim)`` (connectivity
  26) or ``(ndim, 1)`` (6), ``bincount`` of the labels, every component below ``min_size`` becomes ``background_label``;
* holes: ``ndimage.binary_fill_holes(seg in S) & ~(seg in S)`` with scipy's default structure, on the array as it is (a 2-D
  map is a 2-D array); hole voxels whose value is ``background_label`` become ``fill_label``.
"""
import numpy as np
from scipy import ndimage


def set_of(labels_or_regions):
    members = labels_or_regions if isinstance(labels_or_regions, list) else [labels_or_regions]
    out = set()
    for m in members:
        out.update([int(m)] if np.isscalar(m) else [int(v) for v in m])
    return sorted(out)


def small_components_of_set(seg, values, min_size, connectivity=26):
    """The mask of the voxels that one set loses, and nothing else."""
    seg = np.asarray(seg)
    mask = np.isin(seg, values)
    structure = ndimage.generate_binary_structure(seg.ndim, seg.ndim if connectivity == 26 else 1)
    lab, n = ndimage.label(mask, structure=structure)
    if n == 0:
        return np.zeros(seg.shape, bool)
    sizes = np.bincount(lab.ravel(), minlength=n + 1)
    small = sizes < min_size
    small[0] = False
    return small[lab]


def remove_small_ref(seg, labels_or_regions, min_size, background_label=0, connectivity=26, per_member=False):
    """``remove_small_components_from_segmentation``: with ``per_member`` every member of the list is a set of its own, all
    labelled on the input map."""
    seg = np.asarray(seg)
    if per_member and isinstance(labels_or_regions, list):
        sets = [set_of(m) for m in labels_or_regions]
    else:
        sets = [set_of(labels_or_regions)]
    sizes = list(min_size) if isinstance(min_size, (list, tuple, np.ndarray)) else [min_size] * len(sets)
    out = np.copy(seg)
    for values, m in zip(sets, sizes):
        out[small_components_of_set(seg, values, m, connectivity)] = background_label
    return out


def holes_of(mask):
    """scipy's holes of a boolean mask of any rank (its own border rule: a (1, Y, Z) array has no hole)."""
    mask = np.asarray(mask, bool)
    if mask.size == 0:
        return np.zeros(mask.shape, bool)
    return ndimage.binary_fill_holes(mask) & ~mask


def fill_holes_ref(seg, labels_or_regions, fill_label=None, background_label=0):
    seg = np.asarray(seg)
    values = set_of(labels_or_regions)
    if fill_label is None:
        assert len(values) == 1
        fill_label = values[0]
    out = np.copy(seg)
    out[holes_of(np.isin(seg, values)) & (seg == background_label)] = fill_label
    return out


def keep_largest_ref(seg, labels_or_regions, background_label=0):
    """The largest-component step (tests/test_postprocessing_cpu.py's restatement), for mixed lists."""
    seg = np.asarray(seg)
    mask = np.isin(seg, set_of(labels_or_regions))
    lab, n = ndimage.label(mask, structure=ndimage.generate_binary_structure(seg.ndim, seg.ndim))
    out = np.copy(seg)
    if n:
        sizes = np.bincount(lab.ravel())[1:]
        out[mask & ~np.isin(lab, np.flatnonzero(sizes == sizes.max()) + 1)] = background_label
    return out


def apply_ref(seg, steps):
    """``steps``: a list of ``(kind, kwargs)`` with kind 'largest', 'small' or 'holes', or ``(callable, kwargs)``; applied in order."""
    fns = {'largest': keep_largest_ref, 'small': remove_small_ref, 'holes': fill_holes_ref}
    for kind, kw in steps:
        seg = fns[kind](seg, **kw) if isinstance(kind, str) else np.asarray(kind(np.copy(seg), **kw))
    return seg


# ---- hand-made maps, the answer written out -------------------------------------------------------------------------
def _shell(a, lo, hi, value):
    """The faces of the cube [lo, hi] (inclusive) of a 3-D array get ``value``."""
    s = slice(lo, hi + 1)
    for ax in range(3):
        for side in (lo, hi):
            idx = [s, s, s]
            idx[ax] = side
            a[tuple(idx)] = value


def hole_cases():
    """(name, seg, kwargs of fill_holes, expected)."""
    out = []
    # a closed cube shell with a one-voxel cavity: filled
    a = np.zeros((5, 5, 5), np.uint8)
    _shell(a, 1, 3, 1)
    e = a.copy(); e[2, 2, 2] = 1
    out.append(('cavity', a, dict(labels_or_regions=[1]), e))
    # 2-D ring whose only gap is closed diagonally: the cross structure does not pass a diagonal, so it is still a hole
    b = np.zeros((5, 5), np.uint8)
    b[1, 1:4] = 1; b[3, 1:4] = 1; b[2, 1] = 1; b[2, 3] = 1
    b[1, 3] = 0                                             # the ring's corner is missing: (2, 2) touches (1, 3) only diagonally
    e = b.copy(); e[2, 2] = 1
    out.append(('diagonal_gap_2d', b, dict(labels_or_regions=[1]), e))
    # the same in 3-D: a shell with one corner voxel missing is still closed for face neighbours
    c = np.zeros((5, 5, 5), np.uint8)
    _shell(c, 1, 3, 1)
    c[1, 1, 1] = 0
    e = c.copy(); e[2, 2, 2] = 1
    out.append(('diagonal_gap_3d', c, dict(labels_or_regions=[1]), e))
    # a one-voxel tunnel through the shell's face and on to the border opens the cavity: nothing changes
    d = np.zeros((6, 5, 5), np.uint8)
    _shell(d, 1, 3, 1)
    d[3, 2, 2] = 0                                          # the face's centre: cavity - tunnel - (4, 2, 2) - border (5, 2, 2)
    out.append(('tunnel', d, dict(labels_or_regions=[1]), d.copy()))
    # another label inside the hole stays, the background around it is filled
    f = np.zeros((7, 7, 7), np.uint8)
    _shell(f, 1, 5, 1)
    f[3, 3, 3] = 2
    e = f.copy(); e[2:5, 2:5, 2:5] = 1; e[3, 3, 3] = 2
    out.append(('label_inside', f, dict(labels_or_regions=[1]), e))
    # a shell inside a hole inside a shell: everything inside the outer shell is a hole of the set
    g = np.zeros((9, 9, 9), np.uint8)
    _shell(g, 1, 7, 1)
    _shell(g, 3, 5, 1)
    e = g.copy(); e[2:7, 2:7, 2:7] = 1
    out.append(('shell_in_shell', g, dict(labels_or_regions=[1]), e))
    # a region (tuple) with an explicit fill label and a background other than 0
    h = np.full((5, 5, 5), 7, np.uint8)
    _shell(h, 1, 3, 1)
    h[1, 2, 2] = 2                                          # the shell is made of labels 1 and 2
    e = h.copy(); e[2, 2, 2] = 9
    out.append(('region_fill_9_background_7', h, dict(labels_or_regions=[(1, 2)], fill_label=9, background_label=7), e))
    return out


def small_cases():
    """(name, seg, kwargs of remove_small, expected)."""
    out = []
    a = np.zeros((4, 6, 6), np.uint8)
    a[0, 0, 0:3] = 1                                        # 3 voxels: exactly min_size, kept
    a[2, 3, 0:2] = 1                                        # 2 voxels: min_size - 1, removed
    a[3, 5, 5] = 2                                          # another label: not in the set
    e = a.copy(); e[2, 3, 0:2] = 0
    out.append(('exactly_min_size', a, dict(labels_or_regions=[1], min_size=3), e))
    b = np.zeros((4, 4, 4), np.uint8)
    b[0, 0, 0:2] = 1; b[1, 1, 2:4] = 1                      # two blobs of 2 that touch at a corner: (0,0,1) - (1,1,2)
    out.append(('corner_26_one_component', b, dict(labels_or_regions=[1], min_size=4, connectivity=26), b.copy()))
    out.append(('corner_6_two_components', b, dict(labels_or_regions=[1], min_size=4, connectivity=6), np.zeros_like(b)))
    c = np.zeros((3, 5, 5), np.uint8)
    c[0, 0, 0] = 1; c[0, 0, 1] = 2                          # together 2 voxels, each alone 1
    c[2, 4, 4] = 2
    e = c.copy(); e[2, 4, 4] = 0
    out.append(('union_of_members', c, dict(labels_or_regions=[1, 2], min_size=2), e))
    out.append(('per_member', c, dict(labels_or_regions=[1, 2], min_size=2, per_member=True), np.zeros_like(c)))
    e = c.copy(); e[0, 0, 0] = 0
    out.append(('per_member_sizes', c, dict(labels_or_regions=[1, 2], min_size=[2, 1], per_member=True), e))
    d = np.full((3, 4, 4), 5, np.uint8)
    d[1, 1, 1] = 1
    e = d.copy(); e[1, 1, 1] = 5
    out.append(('background_5', d, dict(labels_or_regions=1, min_size=2, background_label=5), e))
    out.append(('min_size_1_is_a_no_op', d, dict(labels_or_regions=1, min_size=1, background_label=5), d.copy()))
    out.append(('min_size_0_is_a_no_op', d, dict(labels_or_regions=1, min_size=0, background_label=5), d.copy()))
    return out
