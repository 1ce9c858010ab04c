"""The yardstick of the surface-distance tests, in plain numpy (no scipy, no GPU, no test in here).

For a boolean mask M on a (z, y, x) grid: the surface S(M) = M & ~erode(M), one step of binary erosion with the
6-neighbourhood, everything outside the volume being background.  The directed distances d(A -> B): for every voxel a of
S(A) in raster order, sqrt(min over b in S(B) of ((sz dz)^2 + (sy dy)^2) + (sx dx)^2) - float64, the sum taken in exactly
that order, the minimum over the evaluated values, so that no traversal order can change a bit.
tests/test_surface_ref_cpu.py holds this against scipy's binary_erosion and distance_transform_edt."""
import numpy as np

KEYS = ('HD', 'HD95', 'ASSD', 'NSD', 'n_surf_pred', 'n_surf_ref')


def surface(mask) -> np.ndarray:
    """M & ~erode(M): six shifted ANDs, the volume's faces eroded."""
    m = np.asarray(mask, dtype=bool)
    inner = m.copy()
    for ax in range(m.ndim):
        lo = [slice(None)] * m.ndim
        hi = [slice(None)] * m.ndim
        lo[ax], hi[ax] = slice(0, -1), slice(1, None)
        lo, hi = tuple(lo), tuple(hi)
        before = np.zeros_like(m)               # the neighbour at -1 along ax, background outside
        before[hi] = m[lo]
        after = np.zeros_like(m)                # the neighbour at +1
        after[lo] = m[hi]
        inner &= before & after
    return m & ~inner


def region_mask(seg, label_or_region) -> np.ndarray:
    members = [label_or_region] if np.isscalar(label_or_region) else list(label_or_region)
    return np.isin(np.asarray(seg), members)


def sq_distances(a, b, spacing, pairs: int = 1 << 21) -> np.ndarray:
    """The squared d(a -> b) of two boolean masks, brute force over the coordinates of both surfaces, ``pairs`` at a time."""
    pa = np.argwhere(surface(a)).astype(np.float64).T           # raster order; rows z, y, x
    pb = np.argwhere(surface(b)).astype(np.float64).T
    sz, sy, sx = (np.float64(s) for s in spacing)
    n_a, n_b = pa.shape[1], pb.shape[1]
    if n_b == 0:
        return np.full(n_a, np.inf)
    out = np.empty(n_a, np.float64)
    chunk = max(1, pairs // n_b)
    for k in range(0, n_a, chunk):
        az, ay, ax = (np.ascontiguousarray(c[k:k + chunk])[:, None] for c in pa)
        t = (sz * (az - pb[0][None, :])) ** 2
        t += (sy * (ay - pb[1][None, :])) ** 2                   # ((sz dz)^2 + (sy dy)^2) ...
        t += (sx * (ax - pb[2][None, :])) ** 2                   # ... + (sx dx)^2
        out[k:k + chunk] = t.min(axis=1)
    return out


def box(mask):
    """[lo, hi) per axis of a boolean mask as (lo_z, hi_z, lo_y, hi_y, lo_x, hi_x); zeros for an empty one."""
    at = np.argwhere(mask)
    if len(at) == 0:
        return [0] * 6
    return [int(v) for ax in range(3) for v in (at[:, ax].min(), at[:, ax].max() + 1)]


def metrics(dp, dr, n_p, n_r, tolerance) -> dict:
    """medpy's hd, hd95, assd and the normalised surface Dice from the directed distances (not squared)."""
    out = {}
    if n_p == 0 or n_r == 0:
        out['HD'] = out['HD95'] = out['ASSD'] = out['NSD'] = np.nan
    else:
        out['HD'] = max(dp.max(), dr.max())
        out['HD95'] = np.percentile(np.hstack((dp, dr)), 95)
        out['ASSD'] = np.mean((dp.mean(), dr.mean()))
        out['NSD'] = ((dp <= tolerance).sum() + (dr <= tolerance).sum()) / (n_p + n_r)
    out['n_surf_pred'] = n_p
    out['n_surf_ref'] = n_r
    return out


def case(seg_ref, seg_pred, labels_or_regions, spacing):
    """What fnn_surface_count and fnn_surface_distances must give for two label maps: (n_surface [R, 2] = |S(ref_r)|,
    |S(pred_r)|; boxes [R, 6] of ref_r | pred_r; the sq_dist buffer - per region with two non-empty sides the squared
    d(pred -> ref), then d(ref -> pred))."""
    n_surface, boxes, parts = [], [], []
    for r in labels_or_regions:
        mr, mp = region_mask(seg_ref, r), region_mask(seg_pred, r)
        n_r, n_p = int(surface(mr).sum()), int(surface(mp).sum())
        n_surface.append([n_r, n_p])
        boxes.append(box(mr | mp))
        if n_r and n_p:
            parts += [sq_distances(mp, mr, spacing), sq_distances(mr, mp, spacing)]
    return (np.array(n_surface, np.int64).reshape(-1, 2), np.array(boxes, np.int64).reshape(-1, 6),
            np.concatenate(parts) if parts else np.zeros(0, np.float64))


def case_metrics(seg_ref, seg_pred, labels_or_regions, spacing, tolerance=1.0) -> dict:
    out = {}
    for r in labels_or_regions:
        mr, mp = region_mask(seg_ref, r), region_mask(seg_pred, r)
        n_r, n_p = int(surface(mr).sum()), int(surface(mp).sum())
        if n_r and n_p:
            dp, dr = np.sqrt(sq_distances(mp, mr, spacing)), np.sqrt(sq_distances(mr, mp, spacing))
        else:
            dp = dr = np.zeros(0)
        out[r] = metrics(dp, dr, n_p, n_r, tolerance)
    return out
