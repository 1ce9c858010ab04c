"""The yardstick of the lesion-wise metrics: the definitions stated with ``scipy.ndimage.label(mask, np.ones((3, 3, 3)))``
(26-connectivity, outside the volume is background) and numpy, nothing shared with the package.

For one label or region r: P_1..P_m are the components of the prediction's mask, R_1..R_n those of the reference's, both
numbered by their first voxel in raster order; o(i, j) = |P_i & R_j|."""
import numpy as np
from scipy import ndimage

KEYS = ('n_inst_ref', 'n_inst_pred', 'inst_TP', 'inst_FN', 'inst_FP', 'inst_recall', 'inst_precision', 'inst_F1',
        'FN_inst_vox', 'FP_inst_vox', 'PQ', 'SQ', 'RQ')
FULL = np.ones((3, 3, 3), int)


def region_mask(seg, r):
    return np.isin(np.asarray(seg), [int(v) for v in (r if isinstance(r, (tuple, list)) else (r,))])


def components(mask):
    """(ids int32 like mask: 0 outside, k + 1 in component k; first voxels int64 [n] as raster indices; sizes int64 [n]).
    scipy numbers the components in the order it meets them in a raster scan - by first voxel; asserted here."""
    mask = np.asarray(mask, bool)
    ids, n = ndimage.label(mask, FULL)
    flat = ids.reshape(-1)
    where = np.flatnonzero(flat)
    uniq, first = np.unique(flat[where], return_index=True)
    roots = where[first].astype(np.int64)
    assert list(uniq) == list(range(1, n + 1)) and np.all(np.diff(roots) > 0), 'scipy.ndimage.label: not in first-voxel order'
    return ids, roots, np.bincount(flat, minlength=n + 1)[1:].astype(np.int64)


def overlaps(ref, pred, r):
    """{'ref_sizes', 'pred_sizes', 'pairs', 'ref_roots', 'pred_roots'} of one label or region; pairs int64 [k, 3] =
    (pred index, ref index, o), every pair with o > 0, sorted by the indices."""
    ref_ids, ref_roots, ref_sizes = components(region_mask(ref, r))
    pred_ids, pred_roots, pred_sizes = components(region_mask(pred, r))
    both = (ref_ids > 0) & (pred_ids > 0)
    pi, ri = pred_ids[both].astype(np.int64) - 1, ref_ids[both].astype(np.int64) - 1
    n = max(len(ref_sizes), 1)
    key, count = np.unique(pi * n + ri, return_counts=True)
    pairs = np.stack([key // n, key % n, count], axis=1).astype(np.int64).reshape(-1, 3)
    return {'ref_sizes': ref_sizes, 'pred_sizes': pred_sizes, 'pairs': pairs, 'ref_roots': ref_roots, 'pred_roots': pred_roots}


def pieces(ref, pred, regions):
    """The pieces of disjoint regions in one joint map: int64 [k, 4] = (own first voxel, first voxel of the piece's component
    in the prediction, in the reference, size), ascending in the first column."""
    out = []
    for r in regions:
        mr, mp = region_mask(ref, r), region_mask(pred, r)
        _, ref_roots, _ = components(mr)
        _, pred_roots, _ = components(mp)
        ref_ids, pred_ids = ndimage.label(mr, FULL)[0].reshape(-1), ndimage.label(mp, FULL)[0].reshape(-1)
        _, roots, sizes = components(mr & mp)
        out += [(v, pred_roots[pred_ids[v] - 1], ref_roots[ref_ids[v] - 1], s) for v, s in zip(roots, sizes)]
    return np.array(sorted(out), np.int64).reshape(-1, 4)


def records(ref, pred, regions):
    """What fnn_instance_overlaps writes for pairwise disjoint ``regions`` (set g = regions[g]): (n_out int64 [3], records
    int32 [sum, 3]) - the reference's components, then the prediction's, as (set, first voxel, size) ascending in the first
    voxel, then the pieces as (first voxel of their component in the prediction, in the reference, size) ascending in their own."""
    sides = []
    for seg in (ref, pred):
        rows = []
        for g, r in enumerate(regions):
            _, roots, sizes = components(region_mask(seg, r))
            rows += [(int(v), g, int(s)) for v, s in zip(roots, sizes)]
        sides.append(np.array([(g, v, s) for v, g, s in sorted(rows)], np.int64).reshape(-1, 3))
    p = pieces(ref, pred, regions)[:, 1:]
    n_out = np.array([len(sides[0]), len(sides[1]), len(p)], np.int64)
    return n_out, np.concatenate(sides + [p]).astype(np.int32)


def metrics(ref_sizes, pred_sizes, pairs):
    """The table of the definitions, one line each, with Python loops over the components."""
    n, m = len(ref_sizes), len(pred_sizes)
    o = {(int(i), int(j)): int(v) for i, j, v in pairs if v > 0}
    detected = [any((i, j) in o for i in range(m)) for j in range(n)]
    touching = [any((i, j) in o for j in range(n)) for i in range(m)]
    tp, fp = sum(detected), m - sum(touching)
    recall = np.float64(tp) / np.float64(n) if n else np.float64(np.nan)
    precision = np.float64(m - fp) / np.float64(m) if m else np.float64(np.nan)
    if np.isnan(recall) or np.isnan(precision):
        f1 = np.float64(np.nan)
    elif precision + recall == 0:
        f1 = np.float64(0.0)
    else:
        f1 = 2 * precision * recall / (precision + recall)
    out = {'n_inst_ref': np.int64(n), 'n_inst_pred': np.int64(m), 'inst_TP': np.int64(tp), 'inst_FN': np.int64(n - tp),
           'inst_FP': np.int64(fp), 'inst_recall': recall, 'inst_precision': precision, 'inst_F1': f1,
           'FN_inst_vox': np.int64(sum(int(s) for s, d in zip(ref_sizes, detected) if not d)),
           'FP_inst_vox': np.int64(sum(int(s) for s, t in zip(pred_sizes, touching) if not t))}
    if n == 0 and m == 0:
        out['PQ'] = out['SQ'] = out['RQ'] = np.float64(np.nan)
        return out
    ious = []
    for (i, j), v in sorted(o.items()):
        iou = np.float64(v) / np.float64(int(pred_sizes[i]) + int(ref_sizes[j]) - v)
        if iou > 0.5:
            ious.append(iou)
    q = len(ious)
    rq = np.float64(q) / np.float64(q + 0.5 * (m - q) + 0.5 * (n - q))
    sq = np.mean(np.array(ious, np.float64)) if q else np.float64(0.0)
    out['PQ'] = sq * rq
    out['SQ'] = sq
    out['RQ'] = rq
    return out


def case_metrics(ref, pred, regions):
    out = {}
    for r in regions:
        lists = overlaps(ref, pred, r)
        out[r] = metrics(lists['ref_sizes'], lists['pred_sizes'], lists['pairs'])
    return out


def same_value(a, b):
    a, b = float(a), float(b)
    return (np.isnan(a) and np.isnan(b)) or a == b


# ---- maps by construction
def sparse_pair(shape, seed, density=0.03, labels=(1, 2, 3), dtype=np.uint8):
    """``labels`` at ``density`` each (0.03 is well below the 26-neighbour percolation threshold: hundreds of small
    components, not one); the prediction is the reference with a random 30 % of its voxels cleared, rolled by one voxel along
    the fastest axis."""
    rng = np.random.default_rng(seed)
    ref = np.zeros(shape, dtype)
    for v in labels:
        ref[rng.random(shape) < density] = v
    pred = ref.copy()
    pred[rng.random(shape) < 0.3] = 0
    return ref, np.roll(pred, 1, axis=2)


def ring_and_arcs(shape=(1, 9, 9), at=(0, 0, 0), label=1, dtype=np.uint8):
    """A square ring of 24 voxels in the reference; in the prediction its top and its bottom row, each without its middle
    voxel and bridged over the gap outside the ring: one component against two of 9 voxels, two pieces of 3 voxels per pair."""
    ref, pred = np.zeros(shape, dtype), np.zeros(shape, dtype)
    z, y, x = at
    ref[z, y + 1:y + 8, x + 1:x + 8] = label
    ref[z, y + 2:y + 7, x + 2:x + 7] = 0
    for row, bridge in ((y + 1, y), (y + 7, y + 8)):
        pred[z, row, x + 1:x + 8] = label
        pred[z, row, x + 4] = 0
        pred[z, bridge, x + 3:x + 6] = label
    return ref, pred
