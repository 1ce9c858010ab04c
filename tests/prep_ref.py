"""Plain numpy / scipy references and the committed cases for the whole-volume kernels of csrc/prep.hip (bbox, mask_init,
mask_sweep, stats, apply, revert) and for the edge shapes of csrc/resample.hip.  No device code at import.

tests/test_gpu_prep_ops.py runs the cases on the device; tests/test_prep_ref_cpu.py proves without a GPU that every case
discriminates (a reference with the mistake the case is meant to catch gives another answer).

Conventions: `raw` is what the C ABI takes, float32 [C, X, Y, Z] in the file's axis order; `raw_t` is the same data with
transpose_forward applied to its spatial axes (transposed axis a = raw axis tf[a]).  Every generator builds its volume in
transposed coordinates, where the box and the mask live, and hands it over through `to_raw`."""
import itertools
import math

import numpy as np
from scipy import ndimage as ndi

PERMS = list(itertools.permutations(range(3)))
THREE_PERMS = [(0, 1, 2), (2, 0, 1), (1, 0, 2)]

BBOX_STRIDE = 256 * 32 * 256          # voxels one trip of bbox_kernel's grid covers
STATS_STRIDE = 256 * 16 * 256         # ... of stats_kernel's
MINMAX_STRIDE = 2048 * 256            # ... of resample.hip's minmax_kernel, per channel or slice
SWEEP_CAP = 4096                      # the iteration bound fnn_preprocess used to leave silently


def transpose_raw(raw, tf):
    return raw.transpose([0, *[1 + int(i) for i in tf]])


def to_raw(raw_t, tf):
    """The contiguous raw volume whose transpose_forward view is raw_t."""
    tb = np.argsort(tf)
    return np.ascontiguousarray(raw_t.transpose([0, *[1 + int(i) for i in tb]]))


# ---- references ---------------------------------------------------------------------------------------------------------
def nonzero_any(raw_t):
    return (raw_t != 0).any(0)                                   # -0.0 != 0 is False, NaN != 0 is True


def filled_mask(raw_t):
    """create_nonzero_mask: any channel != 0, holes filled (6-connected background that cannot reach the border)."""
    return ndi.binary_fill_holes(nonzero_any(raw_t))


def bbox(raw, tf):
    """[[lo, hi], ...] per transposed axis of the voxels where any channel is non-zero; the full extent for none."""
    nz = nonzero_any(transpose_raw(raw, tf))
    out = []
    for ax in range(3):
        idx = np.flatnonzero(nz.any(axis=tuple(a for a in range(3) if a != ax)))
        out.append([int(idx[0]), int(idx[-1]) + 1] if idx.size else [0, int(nz.shape[ax])])
    return out


def crop(raw, tf, box):
    return transpose_raw(raw, tf)[(slice(None), *[slice(lo, hi) for lo, hi in box])]


def stats64(x):
    """Mean and population std of an fp32 array: exactly rounded float64 sums (math.fsum), the mean first and the squared
    deviations about it second."""
    v = np.asarray(x, np.float32).astype(np.float64).ravel()
    mean = math.fsum(v.tolist()) / v.size
    return mean, math.sqrt(math.fsum(((v - mean) ** 2).tolist()) / v.size)


def apply32(x, a, b):
    """apply_kernel's arithmetic: an fp32 subtraction and an fp32 division, two roundings."""
    return ((np.asarray(x, np.float32) - np.float32(a)) / np.float32(b)).astype(np.float32)


def _neighbours32(v):
    v = np.float32(v)
    return [np.nextafter(v, np.float32(-np.inf)), v, np.nextafter(v, np.float32(np.inf))]


def zscore_candidates(x, mask=None):
    """The nine outputs apply32(x, a', b') with a' in {fl32(mean64) and its two fp32 neighbours} and b' likewise around
    fl32(std64), statistics over x[mask]; voxels outside the mask are untouched.  -> [((a', b'), array), ...]"""
    x = np.asarray(x, np.float32)
    inside = np.ones(x.shape, bool) if mask is None else mask
    mean, std = stats64(x[inside])
    out = []
    for a in _neighbours32(mean):
        for b in _neighbours32(std):
            y = x.copy()
            y[inside] = apply32(x[inside], a, b)
            out.append(((a, b), y))
    return out


def zscore_truth64(x):
    mean, std = stats64(x)
    return (np.asarray(x, np.float32).astype(np.float64) - mean) / std


def sweep_model(nz):
    """Synchronous model of mask_init_kernel + the mask_sweep_kernel iterations on the box `nz` (True = some channel
    non-zero): background on a box face starts outside; one iteration sweeps axis 0, 1, 2 in turn, and a sweep turns a
    whole run of background along its axis outside when the run holds an outside voxel or a voxel with an outside side
    neighbour, all read from the state the sweep started with.
    -> (iterations that changed the mask, the filled mask)."""
    bg = ~nz
    face = np.zeros(nz.shape, bool)
    for ax in range(3):
        sl = [slice(None)] * 3
        for end in (0, -1):
            sl[ax] = end
            face[tuple(sl)] = True
    out = bg & face
    runs = []
    for ax in range(3):
        st = np.zeros((3, 3, 3), bool)
        st[1, 1, 1] = True
        sl = [1, 1, 1]
        for d in (0, 2):
            sl[ax] = d
            st[tuple(sl)] = True
            sl[ax] = 1
        runs.append(ndi.label(bg, structure=st)[0])
    its = 0
    while True:
        before = int(out.sum())
        for ax in range(3):
            seed = out.copy()
            for side in range(3):
                if side == ax:
                    continue
                for sh in (1, -1):
                    nb = np.roll(out, sh, axis=side)
                    sl = [slice(None)] * 3
                    sl[side] = 0 if sh == 1 else -1
                    nb[tuple(sl)] = False
                    seed |= nb
            hit = np.unique(runs[ax][seed & bg])
            out = bg & np.isin(runs[ax], hit[hit > 0])
        if int(out.sum()) == before:
            return its, ~out
        its += 1


# ---- (a) box cases ------------------------------------------------------------------------------------------------------
BBOX_SHAPE = (2, 17, 23, 29)
BBOX_CASES = ['ragged', 'single_voxel', 'all_zero', 'face_0lo', 'face_0hi', 'face_1lo', 'face_1hi', 'face_2lo', 'face_2hi',
              'channel_1_only', 'negative_zero_only', 'single_nan']


def bbox_case(name):
    """raw [2, 17, 23, 29] in file order (the test runs it under all six permutations)."""
    rng = np.random.default_rng(BBOX_CASES.index(name) + 100)
    raw = np.zeros(BBOX_SHAPE, np.float32)
    if name == 'ragged':                                        # sparse, so every face of the box is set by a few voxels
        core = rng.random((2, 11, 18, 20)) < 0.02
        raw[:, 4:15, 0:18, 6:26][core] = 1.5
    elif name == 'single_voxel':
        raw[0, 16, 0, 13] = -2.0
    elif name.startswith('face_'):
        raw[:, 7:10, 9:13, 11:16] = rng.standard_normal((2, 3, 4, 5)).astype(np.float32) + 3
        ax, end = int(name[5]), name[6:]
        at = [8, 10, 12]
        at[ax] = 0 if end == 'lo' else BBOX_SHAPE[1 + ax] - 1
        raw[(1, *at)] = 1e-30
    elif name == 'channel_1_only':
        raw[1, 2:9, 20:22, 3:4] = 7.0
    elif name == 'negative_zero_only':
        raw[:] = -0.0
    elif name == 'single_nan':
        raw[:] = -0.0
        raw[1, 5, 22, 28] = np.nan
    return raw


def bbox_stride_case():
    """[1, 132, 128, 128]: non-zero only past the first trip of bbox_kernel's grid-stride loop."""
    raw = np.zeros((1, 132, 128, 128), np.float32)
    for at in ((129, 5, 7), (131, 100, 90), (130, 64, 127)):
        raw[(0, *at)] = 1.0
    return raw


# ---- (b) mask cases -----------------------------------------------------------------------------------------------------
def _embed(box_t, margins):
    """The box inside an image with zero margins ((lo, hi) per transposed axis; 0 = that box face is the image border)."""
    shape = [box_t.shape[0]] + [lo + n + hi for n, (lo, hi) in zip(box_t.shape[1:], margins)]
    img = np.zeros(shape, np.float32)
    img[(slice(None), *[slice(lo, lo + n) for n, (lo, hi) in zip(box_t.shape[1:], margins)])] = box_t
    return img


def _values(rng, shape):
    return (rng.random(shape) + 1).astype(np.float32)          # in [1, 2): the mean is far from zero


MARGINS = [((0, 0), (0, 0), (0, 0)), ((2, 0), (0, 3), (1, 1)), ((0, 1), (4, 0), (0, 0))]
PERCOLATION_SHAPES = [(1, 37, 53), (2, 30, 41), (3, 300, 7), (40, 44, 36)]
PERCOLATION_FRACTIONS = [0.25, 0.31, 0.40]
# shape x zero fraction; channels, permutation and margins cycle so that each occurs with every shape
PERCOLATION_CASES = [dict(shape=s, zero=f, channels=1 + (i + j) % 2, tf=THREE_PERMS[(i + j) % 3], margins=MARGINS[(i + 2 * j) % 3],
                          seed=10 * i + j)
                     for i, s in enumerate(PERCOLATION_SHAPES) for j, f in enumerate(PERCOLATION_FRACTIONS)]


def percolation_case(case):
    """-> raw_t [C, ...]: a random map on the box whose any-channel mask has the case's zero fraction (two channels: independent
    zero patterns of fraction sqrt(f) each), the box corners set so that the crop box is the box; half the zeros are -0.0."""
    rng = np.random.default_rng(1000 + case['seed'])
    C, shape = case['channels'], case['shape']
    box = _values(rng, (C, *shape))
    box[rng.random((C, *shape)) < case['zero'] ** (1.0 / C)] = 0
    box[0][tuple(np.ix_(*[[0, n - 1] for n in shape]))] = 1.25
    zeros = np.flatnonzero(box == 0)
    box.ravel()[zeros[::2]] = -0.0
    return _embed(box, case['margins'])


MASK_CASES = ['diagonal_contact', 'face_background_only', 'nan_wall']


def mask_case(name):
    """-> (raw_t [C, ...], schemes per channel); channel 0 is the one the mask is read from."""
    rng = np.random.default_rng(MASK_CASES.index(name) + 200)
    if name == 'diagonal_contact':
        # a zero room that meets outside background only across a corner (5,5,5) and an edge (2,5,4): it stays inside
        box = _values(rng, (1, 9, 9, 9))
        box[0, 3:5, 3:5, 3:5] = 0
        box[0, 5, 5, 5:9] = 0
        box[0, 0:3, 5, 4] = 0
        return box, ['ZScoreNormalization']
    if name == 'face_background_only':
        box = _values(rng, (1, 6, 5, 9))
        face = np.ones((6, 5, 9), bool)
        face[1:-1, 1:-1, 1:-1] = False
        box[0][face & (rng.random((6, 5, 9)) < 0.4)] = 0          # no zero in the interior: nothing for the sweeps to do
        box[0][tuple(np.ix_([0, 5], [0, 4], [0, 8]))] = 1.25
        return _embed(box, MARGINS[1]), ['ZScoreNormalization']
    if name == 'nan_wall':
        # channel 0 is zero in a room and in the wall round it; the wall is NaN in channel 1: NaN != 0, the room is a hole
        box = np.stack([_values(rng, (8, 9, 10)), np.zeros((8, 9, 10), np.float32)])
        box[0, 2:7, 2:7, 2:8] = 0
        box[1, 2:7, 2:7, 2:8] = np.nan
        box[1, 3:6, 3:6, 3:7] = 0
        box[0, 4, 0:2, 5] = 0                                     # a corridor from the face up to the wall
        return box, ['ZScoreNormalization', 'NoNormalization']
    raise KeyError(name)


SERPENTINE_R = 16420                   # R / 4 = 4105 > SWEEP_CAP; the model needs R / 2 iterations


def serpentine(R):
    """-> raw_t [1, 3, R, 5]: all non-zero but a corridor in the middle plane that enters at (1, 0, 3) and crosses the
    box R / 2 times: odd rows are free, even rows are walls with one gap, alternately at column 1 and column 3."""
    box = _values(np.random.default_rng(300), (1, 3, R, 5))
    box[0, 1, 0, 3] = 0
    for r in range(1, R - 1):
        if r % 2:
            box[0, 1, r, 1:4] = 0
        else:
            box[0, 1, r, 1 if r % 4 == 2 else 3] = 0
    return box


# ---- (c) statistics and apply cases -------------------------------------------------------------------------------------
CT_PROPS = {'mean': 50.25, 'std': 33.5, 'percentile_00_5': -100.0, 'percentile_99_5': 200.0}
SCHEME_IDS = {'NoNormalization': 0, 'ZScoreNormalization': 1, 'CTNormalization': 2, 'RescaleTo01Normalization': 3,
              'RGBTo01Normalization': 4}


def norm_desc(scheme, props=None, use_mask=False):
    """The (scheme, mean, std, lower, upper, use_mask) tuple capi.preprocess takes."""
    if scheme == 'CTNormalization':
        return (SCHEME_IDS[scheme], props['mean'], props['std'], props['percentile_00_5'], props['percentile_99_5'], 0)
    return (SCHEME_IDS[scheme], 0., 1., 0., 0., int(use_mask))


def _ct_values(rng, shape):
    x = (rng.standard_normal(shape) * 120 + 40).astype(np.float32)
    x.ravel()[:8] = [-100.0, 200.0, np.nextafter(np.float32(-100), np.float32(-200)), np.nextafter(np.float32(-100), np.float32(0)),
                     np.nextafter(np.float32(200), np.float32(0)), np.nextafter(np.float32(200), np.float32(300)), -1e30, 1e30]
    return x


EXACT_CASES = ['edges', 'std_zero', 'eight_channels', 'stats_stride']


def exact_case(name):
    """-> (raw_t, tf, schemes, props per channel): CT / RescaleTo01 / RGBTo01 / None channels, compared bit for bit."""
    rng = np.random.default_rng(EXACT_CASES.index(name) + 400)
    if name == 'edges':                                          # values at, next to and far beyond lower and upper
        shape = (9, 11, 13)
        box = np.stack([_ct_values(rng, shape), (rng.random(shape) * 4 + 5).astype(np.float32),
                        rng.integers(0, 256, shape).astype(np.float32), rng.standard_normal(shape).astype(np.float32)])
        box[2].ravel()[:2] = [0, 255]
        return (_embed(box, MARGINS[1]), (1, 2, 0), ['CTNormalization', 'RescaleTo01Normalization', 'RGBTo01Normalization', 'NoNormalization'],
                [CT_PROPS, None, None, None])
    if name == 'std_zero':                                       # CT with std 0 and a constant RescaleTo01 channel: / 1e-8
        shape = (5, 6, 7)
        box = np.stack([_ct_values(rng, shape), np.full(shape, 7.5, np.float32)])
        return box, (0, 2, 1), ['CTNormalization', 'RescaleTo01Normalization'], [dict(CT_PROPS, std=0.0), None]
    if name == 'eight_channels':                                 # the API's limit
        shape = (6, 10, 7)
        schemes = ['RescaleTo01Normalization', 'CTNormalization', 'NoNormalization', 'RGBTo01Normalization'] * 2
        box = np.stack([_ct_values(rng, shape) if s == 'CTNormalization' else
                        rng.integers(1, 256, shape).astype(np.float32) if s == 'RGBTo01Normalization' else
                        (rng.standard_normal(shape) * (c + 1) - 3).astype(np.float32) for c, s in enumerate(schemes)])
        props = [dict(CT_PROPS, mean=10.0 * c) if s == 'CTNormalization' else None for c, s in enumerate(schemes)]
        return _embed(box, MARGINS[2]), (2, 1, 0), schemes, props
    if name == 'stats_stride':
        # [2, 70, 130, 120]: RescaleTo01's minimum and maximum lie past the first trip of stats_kernel's grid-stride loop
        shape = (70, 130, 120)
        box = (rng.random((2, *shape)) + 1).astype(np.float32)
        tail = box.reshape(2, -1)[:, STATS_STRIDE:]
        tail[:] = (rng.standard_normal(tail.shape) * 2000 + 6000).astype(np.float32)
        tail[0, 17], tail[0, 4001] = -5000.0, 17000.0
        return box, (0, 1, 2), ['RescaleTo01Normalization', 'ZScoreNormalization'], [None, None]
    raise KeyError(name)


ZSCORE_EXACT_CASES = ['small', 'odd', 'centred', 'stats_stride']


def zscore_exact_case(name):
    """-> (raw_t, tf): well-conditioned ZScore channels (|mean| / std <= 1e3) with enclosed zero rooms and zero margins, run
    masked and unmasked."""
    rng = np.random.default_rng(ZSCORE_EXACT_CASES.index(name) + 500)
    if name == 'stats_stride':
        raw_t, tf, _, _ = exact_case('stats_stride')
        return raw_t[1:], tf
    shape, mean, std, tf = {'small': ((7, 8, 9), 0.3, 2.0, (0, 1, 2)), 'odd': ((33, 19, 27), -40.0, 15.0, (2, 0, 1)),
                            'centred': ((21, 40, 17), 0.5, 3.0, (1, 0, 2))}[name]
    box = (rng.standard_normal((1, *shape)) * std + mean).astype(np.float32)
    box[box == 0] = 1
    box[0, 2:4, 3:6, 2:5] = 0                                    # an enclosed room: inside the mask
    box[0, 0:2, 1, 6:8] = 0                                      # background that reaches a face: outside
    return _embed(box, MARGINS[1]), tf


ILL_CASES = [(3e4, 1.0), (1e6, 1.0), (16384.0, 0.002)]
ILL_SHAPE = (1, 100, 110, 110)


def ill_case(mean, std):
    rng = np.random.default_rng(int(mean) % 1000 + 600)
    return (rng.standard_normal(ILL_SHAPE) * std + mean).astype(np.float32)


def zscore_old_formula(x):
    """fnn_preprocess' statistics before the two-pass variance: E[x^2] - mean^2 from float64 sums."""
    v = np.asarray(x, np.float32).astype(np.float64).ravel()
    mean = v.sum() / v.size
    return mean, math.sqrt(max((v * v).sum() / v.size - mean * mean, 0.0))


NONFINITE_SCHEMES = ['CTNormalization', 'ZScoreNormalization', 'RescaleTo01Normalization', 'RGBTo01Normalization', 'NoNormalization']


def nonfinite_case(scheme, value):
    rng = np.random.default_rng(NONFINITE_SCHEMES.index(scheme) + 700)
    shape = (1, 6, 7, 8)
    x = rng.integers(1, 256, shape).astype(np.float32) if scheme == 'RGBTo01Normalization' else _values(rng, shape) * 30
    x[0, 3, 4, 5] = value
    return x


# ---- (e) resample cases -------------------------------------------------------------------------------------------------
RESAMPLE_EDGE_CASES = [
    # shape (C, ...), new_shape, order, separate axis: axes of length 1 and 2 (2-D datasets arrive as (1, H, W))
    ((1, 1, 20, 22), (1, 31, 17), 3, 0),
    ((1, 1, 20, 22), (1, 31, 17), 3, None),
    ((1, 2, 9, 9), (3, 9, 14), 3, None),
    ((1, 2, 9, 9), (5, 12, 14), 1, 0),
    ((2, 12, 1, 9), (7, 1, 14), 3, 1),
    ((1, 2, 2, 2), (5, 3, 4), 3, None),
]
RESAMPLE_STRIDE = ((1, 84, 80, 80), (40, 37, 90), 3, None)


def resample_stride_input():
    """A +-1000 step block in the last two planes, past the first trip of minmax_kernel's grid-stride loop: the clip range
    of the whole channel is decided there, and the cubic overshoot at the step is what gets clipped."""
    x = (np.random.default_rng(800).standard_normal(RESAMPLE_STRIDE[0]) * 50 + 10).astype(np.float32)
    x[0, 82:, 10:70, 10:40] = 1000.0
    x[0, 82:, 10:70, 40:70] = -1000.0
    return x
