"""The rule of the binary-morphology steps restated with scipy and numpy: what tests/test_morph_cpu.py checks on hand-made
maps and tests/test_gpu_morph.py compares the device results with, bit for bit.

With ``M = seg in S`` and R scipy's ``binary_dilation`` / ``binary_erosion`` / ``binary_opening`` / ``binary_closing`` of M
with ``structure=generate_binary_structure(ndim, rank)`` (connectivity 6 / 18 / 26 = rank 1 / 2 / 3, capped at ndim, which
gives the same structure), ``iterations`` and ``border_value``, on the array as it is (a 2-D map is a 2-D array):

* dilation and closing: voxels of ``R & ~M`` whose value is ``background_label`` become ``fill_label``;
* erosion and opening: voxels of ``M & ~R`` become ``background_label``.
"""
import numpy as np
from scipy import ndimage

OPS = {'dilation': ndimage.binary_dilation, 'erosion': ndimage.binary_erosion, 'opening': ndimage.binary_opening,
       'closing': ndimage.binary_closing}
ADDS = ('dilation', 'closing')
RANK = {6: 1, 18: 2, 26: 3}


def set_of(labels_or_regions):
    members = labels_or_regions if isinstance(labels_or_regions, list) else [labels_or_regions]
    out = set()
    for m in members:
        out.update([int(m)] if np.isscalar(m) else [int(v) for v in m])
    return sorted(out)


def scipy_result(mask, op, iterations=1, connectivity=6, border_value=0):
    """R: scipy's result on a boolean mask of any rank."""
    mask = np.asarray(mask, bool)
    if mask.size == 0:
        return np.zeros(mask.shape, bool)
    assert iterations >= 1
    structure = ndimage.generate_binary_structure(mask.ndim, min(RANK[connectivity], mask.ndim))
    return OPS[op](mask, structure=structure, iterations=int(iterations), border_value=int(border_value))


def morph_ref(seg, op, labels_or_regions, iterations=1, connectivity=6, border_value=0, fill_label=None, background_label=0):
    """``binary_<op>_in_segmentation``; ``op``: 'dilation', 'erosion', 'opening' or 'closing'."""
    seg = np.asarray(seg)
    values = set_of(labels_or_regions)
    m = np.isin(seg, values)
    r = scipy_result(m, op, iterations, connectivity, border_value)
    out = np.copy(seg)
    if op in ADDS:
        if fill_label is None:
            assert len(values) == 1
            fill_label = values[0]
        out[r & ~m & (seg == background_label)] = fill_label
    else:
        assert fill_label is None
        out[m & ~r] = background_label
    return out


# ---- hand-made maps, the answer written out -------------------------------------------------------------------------
def cases():
    """(name, op, seg, kwargs, expected)."""
    out = []
    # a 3x3x3 cube dilated by the cross: every face grows a 3x3 plate (the 7-point-thick octahedral growth) ...
    a = np.zeros((9, 9, 9), np.uint8)
    a[3:6, 3:6, 3:6] = 1
    e = a.copy()
    e[2:7, 3:6, 3:6] = 1; e[3:6, 2:7, 3:6] = 1; e[3:6, 3:6, 2:7] = 1
    out.append(('cube_cross', 'dilation', a, dict(labels_or_regions=[1]), e))
    # ... and by the full structure a 5x5x5 cube; connectivity 18 leaves the 8 corners of that cube out
    e = a.copy(); e[2:7, 2:7, 2:7] = 1
    out.append(('cube_full', 'dilation', a, dict(labels_or_regions=[1], connectivity=26), e))
    e = e.copy()
    for x in (2, 6):
        for y in (2, 6):
            for z in (2, 6):
                e[x, y, z] = 0
    out.append(('cube_18', 'dilation', a, dict(labels_or_regions=[1], connectivity=18), e))
    # two iterations of the cross from one voxel: the octahedron |dx| + |dy| + |dz| <= 2
    b = np.zeros((7, 7, 7), np.uint8)
    b[3, 3, 3] = 1
    g = np.indices(b.shape) - 3
    e = (np.abs(g).sum(0) <= 2).astype(np.uint8)
    out.append(('octahedron_n2', 'dilation', b, dict(labels_or_regions=1, iterations=2), e))
    # a one-voxel bridge between two 3x3x3 blobs is cut by an opening, and the blobs come back whole
    c = np.zeros((5, 5, 11), np.uint8)
    c[1:4, 1:4, 1:4] = 1; c[1:4, 1:4, 7:10] = 1; c[2, 2, 4:7] = 1
    e = c.copy(); e[2, 2, 4:7] = 0
    out.append(('bridge_cut', 'opening', c, dict(labels_or_regions=[1], connectivity=26), e))
    # the erosion alone leaves the two centres
    e = np.zeros_like(c); e[2, 2, 2] = 1; e[2, 2, 8] = 1
    out.append(('blob_centres', 'erosion', c, dict(labels_or_regions=[1], connectivity=26), e))
    # a one-voxel gap between two plates is closed by a closing with the full structure, with an explicit fill label; the
    # cross closes only the gap's centre (its other voxels have a face neighbour that the dilation did not reach)
    d = np.zeros((7, 7, 9), np.uint8)
    d[2:5, 2:5, 2:4] = 1; d[2:5, 2:5, 5:7] = 1
    e = d.copy(); e[2:5, 2:5, 4] = 3
    out.append(('gap_closed_fill_3', 'closing', d, dict(labels_or_regions=[1], connectivity=26, fill_label=3), e))
    e = d.copy(); e[3, 3, 4] = 1
    out.append(('gap_centre_cross', 'closing', d, dict(labels_or_regions=[1]), e))
    # a different label inside the grown zone stays, the background around it takes the set's label
    f = np.zeros((5, 5, 5), np.uint8)
    f[2, 2, 2] = 1; f[2, 2, 3] = 2
    e = f.copy(); e[1, 2, 2] = e[3, 2, 2] = e[2, 1, 2] = e[2, 3, 2] = e[2, 2, 1] = 1
    out.append(('other_label_stays', 'dilation', f, dict(labels_or_regions=[1]), e))
    # a blob that touches the volume's face is eroded from that face with border_value 0 and not with 1
    h = np.zeros((6, 5, 5), np.uint8)
    h[0:4, 1:4, 1:4] = 1
    e = np.zeros_like(h); e[1:3, 2, 2] = 1
    out.append(('face_eroded_border_0', 'erosion', h, dict(labels_or_regions=[1], border_value=0), e))
    e = np.zeros_like(h); e[0:3, 2, 2] = 1
    out.append(('face_kept_border_1', 'erosion', h, dict(labels_or_regions=[1], border_value=1), e))
    # a closing with border_value 0 at the face: scipy's result loses the blob's face layer, the rule adds nothing and removes nothing
    out.append(('closing_at_face', 'closing', h, dict(labels_or_regions=[1], border_value=0), h.copy()))
    # an opening with border_value 1: scipy's result gains the map's outermost layer, the rule adds nothing; the speck inside
    # goes, the one in that layer is part of scipy's result and stays
    k = np.zeros((8, 8, 8), np.uint8)
    k[1:4, 1:4, 1:4] = 1; k[5, 5, 5] = 1; k[7, 6, 4] = 1
    e = k.copy(); e[5, 5, 5] = 0
    out.append(('opening_border_1', 'opening', k, dict(labels_or_regions=[1], connectivity=26, border_value=1), e))
    # background other than 0: erosion writes it, dilation grows only into it
    p = np.full((5, 5, 5), 7, np.uint8)
    p[1:4, 1:4, 1:4] = 1
    e = np.full_like(p, 7); e[2, 2, 2] = 1
    out.append(('erosion_background_7', 'erosion', p, dict(labels_or_regions=1, background_label=7, border_value=1), e))
    q = np.full((5, 5, 5), 7, np.uint8)
    q[2, 2, 2] = 1; q[2, 2, 1] = 0                           # 0 is a label like any other here
    e = q.copy(); e[1, 2, 2] = e[3, 2, 2] = e[2, 1, 2] = e[2, 3, 2] = e[2, 2, 3] = 1
    out.append(('dilation_background_7', 'dilation', q, dict(labels_or_regions=1, background_label=7), e))
    # a region (tuple) with an explicit fill label
    r = np.zeros((5, 5, 7), np.uint16)
    r[2, 2, 2] = 300; r[2, 2, 3] = 301
    e = r.copy()
    for z in (2, 3):
        e[1, 2, z] = e[3, 2, z] = e[2, 1, z] = e[2, 3, z] = 400
    e[2, 2, 1] = e[2, 2, 4] = 400
    out.append(('region_fill_400', 'dilation', r, dict(labels_or_regions=[(300, 301)], fill_label=400), e))
    # a 2-D map: the cross, and the full 3x3 for 18 and 26 alike
    s = np.zeros((5, 6), np.uint8)
    s[2, 2] = 1
    e = s.copy(); e[1, 2] = e[3, 2] = e[2, 1] = e[2, 3] = 1
    out.append(('cross_2d', 'dilation', s, dict(labels_or_regions=[1]), e))
    e = s.copy(); e[1:4, 1:4] = 1
    out.append(('full_2d_18', 'dilation', s, dict(labels_or_regions=[1], connectivity=18), e))
    out.append(('full_2d_26', 'dilation', s, dict(labels_or_regions=[1], connectivity=26), e))
    return out
