"""The stem and fused-producer kernels (csrc/conv3d_thin.hip, conv3d_row.hip) pinned BIT FOR BIT on exact data, op by op.

Every comparison is np.array_equal on fp16 bit patterns (zeros as +0) or on integer statistics; no tolerance.  Every case
names the kernels it must run, in launch order (fnn_op_last_kernels).  The case tables and their data generators are plain
Python (no device code at import): tests/test_stem_fused_ref_cpu.py imports them and proves, without a GPU, that every
committed (case, mode) is unambiguous and exact, that the over-grid cases have more work units than the persistent grid
restated for them, and that mutants of the reference change the expected bits of some committed case.

Every volume is larger than its patches on every side and holds a large sentinel outside them; origins are non-zero and
differ per item.  Modes (stand-alone stem: ident, stats, round; fused: ident (transposed conv only), readout, dense, stats):

  ident    integer x and integer weights on every tap, dyadic bias, different content per item
  stats    operands of {-1, 0, 1}, weights of +-1 (a fused consumer: a few per output channel): the statistics are integers
           small enough for stats_fit_exact
  round    one-hot weights, zero bias; x sweeps fp32 values at fp16 ties and one fp32 ulp either side, in fp16's subnormal
           range and beyond 2048: y == f16(x)
  readout  ordinary random gamma / beta; the consumer's one-hot weights read channel (5 co + 3) % 16 at tap co % taps out of
           the staged tensor, zero padding on every face included (readout-skip: the same channel of the second chunk;
           readout-b, 27 taps: tap (co + 11) % 27 - the taps 16 output channels do not reach in one mode)
  dense    every item holds the same patch content at another origin of a volume of its own inside another sentinel
           (vol_batch_stride != 0); craft_norm then gives fp16-exact (S, H); dense integer weights, dyadic slope

Shapes are the smallest the launch rules admit (launch_stem_mfma, stem_row_ok, row_choose, conv_thin_ok); the rules are
restated next to the tables and checked in the CPU test."""
import collections
import functools
import zlib

import numpy as np
import pytest

import conv_ref as R

pytestmark = pytest.mark.gpu

K3, K133, K313, S1 = (3, 3, 3), (1, 3, 3), (3, 1, 3), (1, 1, 1)
NO_ROW, NO_STEM1, CM = {'FNN_NO_ROW': '1'}, {'FNN_NO_STEM1': '1'}, {'FNN_OP_CHUNK_MAJOR': '1'}
KNOBS = ('FNN_NO_ROW', 'FNN_NO_STEM_ROW', 'FNN_NO_STEM1', 'FNN_OP_CHUNK_MAJOR')
FLIPS = ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1))
ROW_W = {64: 4, 96: 6, 128: 8, 160: 10, 192: 12}                 # row width -> NBLK
ROW_H = (8, 12, 68, 72)             # the minimum; two groups; pick_strips' fallback (one strip of more than 64 rows); two strips of 36
SENTINEL = 24576.0

# kind: 'stem' (fnn_op_stem), 'fstem' / 'ftconv' (fnn_op_conv_fused).  c: the stem's input channels or the low tensor's;
# dims: the patch = the consumer's size; k: the stem's (= the consumer's) kernel or the consumer's; tstride: the transposed
# conv's; grid: the persistent workgroups the case's units must exceed (PERSISTENT_WGS), or 0
Case = collections.namedtuple('Case', 'id kind n c cout dims k tstride kernels knobs modes flips grid')


def _s(id, n, c, cout, dims, k, kernel, knobs=None, modes=('ident', 'stats', 'round'), flips=(FLIPS[0],), grid=0):
    return Case(id, 'stem', n, c, cout, tuple(dims), tuple(k), None, (kernel,), dict(knobs or {}), tuple(modes), tuple(flips), grid)


def _fs(id, n, dims, k, kernels, knobs=None, modes=('readout', 'dense', 'stats'), flips=(FLIPS[0],), grid=0):
    return Case(id, 'fstem', n, 1, 16, tuple(dims), tuple(k), None, tuple(kernels), dict(knobs or {}), tuple(modes), tuple(flips), grid)


def _ft(id, n, lowc, dims, tstride, kernel, knobs=None, modes=('ident', 'readout', 'readout-skip', 'dense', 'stats'), grid=0):
    return Case(id, 'ftconv', n, lowc, 16, tuple(dims), K133, tuple(tstride), (kernel,), dict(knobs or {}), tuple(modes), (FLIPS[0],), grid)


# workgroups of the persistent grids the over-grid cases are written for:
#   stem_row_kernel        conv3d_row.hip launch_stem_row: gx = 256 * wpc, wpc = 8
#   conv_row_stem_kernel   conv3d_row.hip launch_row_stem_t: gx = 256 * per_cu, cap = 3 for NBLK <= 8 (32000 B of LDS at W = 64: five fit)
#   conv_thin_kernel       conv3d_thin.hip launch_thin_w: gx = 256 * per_cu, per_cu = WPS = 2 (conv_thin_ok: two fit)
PERSISTENT_WGS = {'stem_row_kernel': 2048, 'conv_row_stem_kernel': 768, 'conv_thin_kernel': 512}

TILE, TILE1 = (19, 13, 11), (5, 13, 20)            # 2 x 2 x 2 ragged tiles of 16 x 8 x 8; a (1, 3, 3) patch whose width is no row width
STEM_CASES = [
    # ---- stem_mfma1_kernel<Cout / 16, kd>: one input channel, 16 or 32 output channels
    _s('stem1-1-3', 3, 1, 16, TILE, K3, 'stem_mfma1_kernel<1,3>', flips=FLIPS),
    _s('stem1-2-3', 3, 1, 32, TILE, K3, 'stem_mfma1_kernel<2,3>'),
    _s('stem1-1-1', 3, 1, 16, TILE1, K133, 'stem_mfma1_kernel<1,1>'),
    _s('stem1-2-1', 3, 1, 32, TILE1, K133, 'stem_mfma1_kernel<2,1>'),
    # ---- stem_mfma_kernel: three cout blocks; FNN_NO_STEM1; one padded k-step; four k-steps; two channel groups (8 + 3); (3, 1, 3)
    _s('stem-c1-48', 3, 1, 48, TILE, K3, 'stem_mfma_kernel'),
    _s('stem-c1-16-no-stem1', 3, 1, 16, TILE, K3, 'stem_mfma_kernel', NO_STEM1),
    _s('stem-c3-133', 3, 3, 32, TILE1, K133, 'stem_mfma_kernel'),
    _s('stem-c4-333', 3, 4, 32, TILE, K3, 'stem_mfma_kernel', flips=FLIPS),
    _s('stem-c11-333', 3, 11, 16, TILE, K3, 'stem_mfma_kernel'),
    _s('stem-c2-313', 3, 2, 16, TILE, K313, 'stem_mfma_kernel'),
]
# ---- stem_row_kernel<NBLK, 1>: every row width at every strip form; PD = 3, N = 2: 6 .. 12 units
STEM_CASES += [_s(f'stem-row-{w}-{h}', 2, 1, 16, (3, h, w), K133, f'stem_row_kernel<{nb},1>',
                  flips=FLIPS if (w, h) == (96, 72) else (FLIPS[0],)) for w, nb in ROW_W.items() for h in ROW_H]
# more units than the 2048 workgroups at PH = 16 (the smallest PH whose slot rows, ceil(PD / 16) * 2 * 8, reach PD for a long
# PD).  N PD = 7 x 342 = 2394 is the smallest count at which a workgroup's range of two units crosses an ITEM boundary, not
# only planes (CPU test: with 2 x 1035 = 2070 units no range does)
STEM_CASES += [_s('stem-row-over-grid', 7, 1, 16, (342, 16, 64), K133, 'stem_row_kernel<4,1>', modes=('ident', 'stats'), grid=2048)]

FUSED_STEM_CASES = [
    _fs(f'fstem-row-{w}-{h}', 2, (3, h, w), K133, (f'stem_row_kernel<{nb},0>', f'conv_row_stem_kernel<{nb}>'),
        flips=FLIPS if (w, h) == (96, 72) else (FLIPS[(i * len(ROW_H) + j) % 5],))
    for i, (w, nb) in enumerate(ROW_W.items()) for j, h in enumerate(ROW_H)]
FUSED_STEM_CASES += [
    # more units than 768 workgroups: 7 x 128 = 896 planes of one strip, the smallest count with a range across an item boundary
    _fs('fstem-row-over-grid', 7, (128, 16, 64), K133, ('stem_row_kernel<4,0>', 'conv_row_stem_kernel<4>'), modes=('readout', 'stats'), grid=768),
    # ---- tile form: 12 items of 3 x 3 x 5 ragged tiles of 4 x 8 x 8 = 540 tiles for 512 workgroups
    _fs('fstem-thin-1', 12, (9, 17, 33), K133, ('stem_mfma1_kernel<1,1>', 'conv_thin_kernel<1,1,1,1,2>'), NO_ROW, flips=FLIPS, grid=512),
    _fs('fstem-thin-3', 12, (9, 17, 33), K3, ('stem_mfma1_kernel<1,3>', 'conv_thin_kernel<3,1,1,1,2>'), NO_ROW,
        modes=('readout', 'readout-b', 'dense', 'stats'), flips=(FLIPS[0], FLIPS[4]), grid=512),
]

FUSED_TCONV_CASES = [
    _ft('ftconv-thin-4-c16', 12, 16, (9, 18, 34), (1, 2, 2), 'conv_thin_kernel<1,2,2,4,2>', grid=512),
    _ft('ftconv-thin-4-c32', 12, 32, (9, 18, 34), (1, 2, 2), 'conv_thin_kernel<1,2,2,4,2>', grid=512),
    _ft('ftconv-thin-4-c32-cm', 12, 32, (9, 18, 34), (1, 2, 2), 'conv_thin_kernel<1,2,2,4,2>', CM, modes=('dense',), grid=512),
    _ft('ftconv-thin-8-c16', 12, 16, (10, 18, 34), (2, 2, 2), 'conv_thin_kernel<1,2,2,8,2>', grid=512),
    _ft('ftconv-thin-8-c32', 12, 32, (10, 18, 34), (2, 2, 2), 'conv_thin_kernel<1,2,2,8,2>', grid=512),
]
# ---- conv_row_kernel<NBLK, 2, 1>: the five widths, channels-last and chunk-major low; heights over the strip forms
_FT_H = {64: 8, 96: 72, 128: 12, 160: 68, 192: 8}
for _w, _nb in ROW_W.items():
    FUSED_TCONV_CASES += [
        _ft(f'ftconv-row-{_w}', 2, 32, (3, _FT_H[_w], _w), (1, 2, 2), f'conv_row_kernel<{_nb},2,1>'),
        _ft(f'ftconv-row-{_w}-cm', 2, 32, (3, _FT_H[_w], _w), (1, 2, 2), f'conv_row_kernel<{_nb},2,1>', CM, modes=('readout', 'dense')),
    ]
# one width in tile form on the SAME data (ROW_TWIN: the data of the row case): both forms equal the reference, so each other
FUSED_TCONV_CASES += [_ft('ftconv-row-96-no-row', 2, 32, (3, 72, 96), (1, 2, 2), 'conv_thin_kernel<1,2,2,4,2>', NO_ROW)]
ROW_TWIN = {'ftconv-row-96-no-row': 'ftconv-row-96'}

CASES = STEM_CASES + FUSED_STEM_CASES + FUSED_TCONV_CASES
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)

# every kernel form of the family; each is an asserted kernel of some case (the closing test)
REQUIRED_KERNELS = (
    {'stem_mfma_kernel'} | {f'stem_mfma1_kernel<{a},{b}>' for a in (1, 2) for b in (1, 3)} |
    {f'stem_row_kernel<{nb},{s}>' for nb in ROW_W.values() for s in (0, 1)} | {f'conv_row_stem_kernel<{nb}>' for nb in ROW_W.values()} |
    {f'conv_row_kernel<{nb},2,1>' for nb in ROW_W.values()} |
    {'conv_thin_kernel<1,1,1,1,2>', 'conv_thin_kernel<3,1,1,1,2>', 'conv_thin_kernel<1,2,2,4,2>', 'conv_thin_kernel<1,2,2,8,2>'})

# other data where a draw's scale or shift sat on an fp16 rounding boundary (the CPU test: stage_params at margin 4)
SALT = {('fstem-row-96-8', 'readout'): 1, ('fstem-row-96-12', 'readout'): 1, ('fstem-row-96-68', 'readout'): 1, ('fstem-row-96-72', 'readout'): 3,
        ('fstem-row-128-8', 'readout'): 1, ('fstem-row-160-8', 'readout'): 2, ('fstem-row-192-72', 'readout'): 1, ('fstem-thin-1', 'readout'): 256,
        ('fstem-thin-3', 'readout'): 42, ('ftconv-thin-4-c16', 'readout'): 3, ('ftconv-thin-4-c16', 'readout-skip'): 2,
        ('ftconv-thin-4-c32', 'readout'): 9, ('ftconv-thin-4-c32', 'readout-skip'): 5, ('ftconv-thin-8-c16', 'readout'): 2,
        ('ftconv-thin-8-c16', 'readout-skip'): 4, ('ftconv-thin-8-c32', 'readout-skip'): 3, ('ftconv-row-64', 'readout'): 1,
        ('ftconv-row-96-cm', 'readout'): 1, ('ftconv-row-128', 'readout-skip'): 1, ('ftconv-row-128-cm', 'readout'): 2,
        ('ftconv-row-192-cm', 'readout'): 1}
SLOPE = 0.01                         # the network's LeakyReLU slope, for the modes with ordinary norms
DENSE_SLOPE = 0.25


def _seed(*what):
    return zlib.crc32(repr(what).encode()) % (2 ** 31)


def _rs(case, mode):
    cid = ROW_TWIN.get(case.id, case.id)
    return np.random.RandomState(_seed(cid, mode, SALT.get((cid, mode), 0)))


# ---- volumes ---------------------------------------------------------------------------------------------------------------
def place(patches, own):
    """patches [n, C, PD, PH, PW] -> (vol, origins [n, 3]).  own = False: ONE volume [C, X, Y, Z], the patches one behind the
    other along x with one or two sentinel planes between them; own = True: a volume per item [n, C, X, Y, Z], the origin and
    the sentinel's value different per item.  Margins on every side of every patch; everything outside them is the sentinel."""
    n, C, PD, PH, PW = patches.shape
    org = np.empty((n, 3), np.int32)
    if own:
        vol = np.empty((n, C, PD + 4, PH + 6, PW + 7), np.float32)
        for i in range(n):
            org[i] = (1 + i % 3, 1 + (2 * i) % 4, 1 + (3 * i) % 5)
            vol[i] = SENTINEL / 2 + 512.0 * i
            vol[(i, slice(None)) + tuple(slice(o, o + p) for o, p in zip(org[i], (PD, PH, PW)))] = patches[i]
        return vol, org
    x = 2
    for i in range(n):
        org[i] = (x, 1 + (2 * i) % 4, 1 + (3 * i) % 5)
        x += PD + 1 + i % 2
    vol = np.full((C, x + 1, PH + 6, PW + 7), SENTINEL, np.float32)
    for i in range(n):
        vol[(slice(None),) + tuple(slice(o, o + p) for o, p in zip(org[i], (PD, PH, PW)))] = patches[i]
    return vol, org


def round_pool():
    """fp32 values at fp16 ties and one fp32 ulp either side of them, and the fp16 values below them; both signs: subnormals,
    the first normal binade, around 1, the binade of spacing 1 and the five binades beyond 2048"""
    exps = [0, 1, 14, 15, 25, 26, 27, 28, 29, 30]
    bits = np.concatenate([(e << 10) + np.arange(0, 1023, 7) for e in exps]).astype(np.uint16)
    lo = bits.view(np.float16).astype(np.float64)
    hi = (bits + 1).astype(np.uint16).view(np.float16).astype(np.float64)
    tie = ((lo + hi) / 2).astype(np.float32)
    assert (tie.astype(np.float64) == (lo + hi) / 2).all()
    v = np.concatenate([tie, np.nextafter(tie, np.float32(-np.inf)), np.nextafter(tie, np.float32(np.inf)), lo.astype(np.float32)])
    return np.concatenate([v, -v])


# ---- stand-alone stem ------------------------------------------------------------------------------------------------------
def stem_data(case, mode):
    """-> dict(vol, origins, w [cout, C, *k], bias)"""
    rs = _rs(case, mode)
    shape = (case.n, case.c, *case.dims)
    if mode == 'round':
        pool = round_pool()
        x = np.resize(pool[rs.permutation(pool.size)], int(np.prod(shape))).reshape(shape)
        w = np.zeros((case.cout, case.c, *case.k), np.float32)
        for co in range(case.cout):
            w[(co, co % case.c) + tuple(i // 2 for i in case.k)] = 1.0
        bias = None
    elif mode == 'stats':
        x = rs.randint(-1, 2, shape)
        w = rs.choice([-1.0, 1.0], (case.cout, case.c, *case.k))
        bias = 2.0 * rs.randint(-1, 1, case.cout) + 1
    else:
        x = rs.randint(-3, 4, shape)
        w = rs.choice([-2.0, -1.0, 1.0, 2.0], (case.cout, case.c, *case.k))
        bias = (2 * rs.randint(-4, 4, case.cout) + 1) * 0.25
    vol, org = place(x.astype(np.float32), own=False)
    return dict(vol=vol, origins=org, w=w.astype(np.float32), bias=None if bias is None else bias.astype(np.float32))


@functools.lru_cache(maxsize=4)
def stem_reference(cid, mode, flips):
    case = BY_ID[cid]
    d = stem_data(case, mode)
    return d, R.stem_batch(d['vol'], d['origins'], flips, case.dims, d['w'], d['bias'], fast=mode != 'round')


# ---- fused -----------------------------------------------------------------------------------------------------------------
READOUT_TAP0 = {'readout': 0, 'readout-skip': 0, 'readout-b': 11}     # 27 taps: 0 .. 15 and 11 .. 26 - every tap over the two modes


def _one_hot_consumer(cin, k, chunk=0, tap0=0):
    """output channel co reads channel (5 co + 3) % 16 of 16-channel chunk `chunk` at tap (co + tap0) % taps"""
    taps = int(np.prod(k))
    w = np.zeros((16, cin, taps), np.float32)
    for co in range(16):
        w[co, 16 * chunk + (5 * co + 3) % 16, (co + tap0) % taps] = 1.0
    return w.reshape(16, cin, *k)


def _sparse_consumer(rs, cin, k):
    """four weights of +-1 per output channel (mode stats: small integer outputs)"""
    taps = int(np.prod(k))
    w = np.zeros((16, cin * taps), np.float32)
    for co in range(16):
        w[co, rs.choice(cin * taps, 4, replace=False)] = rs.choice([-1.0, 1.0], 4)
    return w.reshape(16, cin, *k)


def _targets(c, off):
    return (np.array([R.F16_TARGETS[(ch + off) % 4][0] for ch in range(c)]), np.array([R.F16_TARGETS[(ch + off) % 4][1] for ch in range(c)]))


def _ordinary_norm(rs, c):
    return (rs.rand(c) + 0.5).astype(np.float32), (rs.randn(c) * 0.3).astype(np.float32)


def fused_stem_data(case, mode, flips):
    """-> dict(vol, origins, sw, sbias, norm, slope, w, bias, stem): stem = the stem's stored values [n, 16, *dims] (the
    reference's), on which craft_norm builds the norm of modes dense / stats.  The stem's operands are small integers in every
    mode, so that its statistics are exact (stats_fit_exact, CPU test) and stage16's bracket of (scale, shift) holds."""
    rs = _rs(case, mode)
    same = mode in ('dense', 'stats')
    x = rs.randint(-1, 2, (1 if same else case.n, 1, *case.dims))
    if same:
        x = np.repeat(x, case.n, 0)
    vol, org = place(x.astype(np.float32), own=same)
    d = dict(vol=vol, origins=org)
    if mode == 'stats':                       # even outputs in [-6, 6]; (S, H) = (0.5, 1): staged integers in [-2, 4]
        sw = np.zeros((16, 9 * case.k[0]), np.float32)
        for co in range(16):
            sw[co, rs.choice(sw.shape[1], 3, replace=False)] = rs.choice([-2.0, 2.0], 3)
        d['sw'], d['sbias'] = sw.reshape(16, 1, *case.k), np.zeros(16, np.float32)
    else:
        d['sw'] = rs.choice([-2.0, -1.0, 1.0, 2.0], (16, 1, *case.k)).astype(np.float32)
        d['sbias'] = rs.randint(-2, 3, 16).astype(np.float32)
    d['stem'] = R.stem_batch(vol, org, flips, case.dims, d['sw'], d['sbias'], fast=True)
    if mode.startswith('readout'):
        d['norm'], d['slope'] = _ordinary_norm(rs, 16), SLOPE
        d['w'], d['bias'] = _one_hot_consumer(16, case.k, tap0=READOUT_TAP0[mode]), None
    elif mode == 'dense':
        d['norm'], d['slope'] = R.craft_norm(d['stem'], *_targets(16, 0)), DENSE_SLOPE
        d['w'] = rs.choice([-2.0, -1.0, 1.0, 2.0], (16, 16, *case.k)).astype(np.float32)
        d['bias'] = ((2 * rs.randint(-4, 4, 16) + 1) * 0.25).astype(np.float32)
    else:
        d['norm'], d['slope'] = R.craft_norm(d['stem'], np.full(16, 0.5), np.full(16, 1.0)), 1.0
        d['w'], d['bias'] = _sparse_consumer(rs, 16, case.k), (2.0 * rs.randint(-1, 1, 16) + 1).astype(np.float32)
    return d


def fused_tconv_data(case, mode):
    """-> dict(low, lnorm, lslope, tw [lowc, 16, *tstride], tbias, skip, snorm, sslope, w [16, 32, 1, 3, 3], bias)"""
    rs = _rs(case, mode)
    s, lc = case.tstride, case.c
    ld = tuple(case.dims[i] // s[i] for i in range(3))
    taps = int(np.prod(s))
    d = dict(lnorm=None, lslope=1.0, snorm=None, sslope=1.0)
    if mode == 'dense':                                                   # test_gpu_conv_exact's norm / two construction
        from test_gpu_conv_exact import SRC_NORM, _permuted_items
        for name, c, dims, (off, slope) in (('low', lc, ld, SRC_NORM[0]), ('skip', 16, case.dims, SRC_NORM[1])):
            first = 2.0 * rs.randint(-4, 5, (c, int(np.prod(dims))))
            x = _permuted_items(first, case.n).reshape(case.n, c, *dims)
            d[name], d[name[0] + 'norm'], d[name[0] + 'slope'] = x.astype(np.float32), R.craft_norm(x, *_targets(c, off)), slope
    else:
        lim = 2 if mode == 'stats' else 4
        d['low'] = rs.randint(1 - lim, lim, (case.n, lc, *ld)).astype(np.float32)
        d['skip'] = rs.randint(1 - lim, lim, (case.n, 16, *case.dims)).astype(np.float32)
    if mode.startswith('readout'):
        d['lnorm'], d['lslope'], d['snorm'], d['sslope'] = _ordinary_norm(rs, lc), SLOPE, _ordinary_norm(rs, 16), SLOPE
        tw = np.zeros((lc, 16, taps), np.float32)                         # phase t of up channel c reads low channel c + t
        for c in range(16):
            for t in range(taps):
                tw[(c + t) % lc, c, t] = 1.0
        d['tw'], d['tbias'] = tw.reshape(lc, 16, *s), None
        d['w'], d['bias'] = _one_hot_consumer(32, K133, chunk=int(mode == 'readout-skip')), None
    elif mode == 'stats':
        tw = np.zeros((lc, 16, taps), np.float32)                         # two low channels per (up channel, phase)
        for c in range(16):
            for t in range(taps):
                tw[rs.choice(lc, 2, replace=False), c, t] = rs.choice([-1.0, 1.0], 2)
        d['tw'], d['tbias'] = tw.reshape(lc, 16, *s), rs.randint(-1, 2, 16).astype(np.float32)
        d['w'], d['bias'] = _sparse_consumer(rs, 32, K133), (2.0 * rs.randint(-1, 1, 16) + 1).astype(np.float32)
    else:
        d['tw'] = rs.choice([-2.0, -1.0, 1.0, 2.0], (lc, 16, *s)).astype(np.float32)
        d['tbias'] = ((2 * rs.randint(-4, 4, 16) + 1) * 0.25).astype(np.float32)
        d['w'] = rs.choice([-2.0, -1.0, 1.0, 2.0], (16, 32, 1, 3, 3)).astype(np.float32)
        d['bias'] = ((2 * rs.randint(-4, 4, 16) + 1) * 0.25).astype(np.float32)
    return d


def fused_staged(case, d, margin=1.0):
    """the tensor the consumer multiplies -> (value, ambiguous)"""
    if case.kind == 'fstem':
        v, _, _, amb = R.fused_stem_staged(d['stem'], d['norm'], d['slope'], margin=margin)
        return v, amb
    return R.fused_tconv_staged(d['low'], d['lnorm'], d['lslope'], d['tw'], d['tbias'], case.tstride, d['skip'], d['snorm'], d['sslope'],
                                margin=margin)


def fused_expected(case, d, a=None):
    a = fused_staged(case, d)[0] if a is None else a
    return R.conv_exact(a, d['w'], d['bias'], case.k, S1, fast=R.fits_exact(a, d['w'], d['bias']))[1]


@functools.lru_cache(maxsize=4)
def fused_reference(cid, mode, flips):
    case = BY_ID[cid]
    d = fused_stem_data(case, mode, flips) if case.kind == 'fstem' else fused_tconv_data(case, mode)
    a, amb = fused_staged(case, d)
    return d, amb, fused_expected(case, d, a)


def units(case):
    """work units of a persistent case: (plane, strip) pairs of the row forms, tiles of 4 x 8 x 8 of the tile form"""
    D, H, W = case.dims
    if case.kernels[-1].startswith('conv_thin_kernel'):
        return case.n * ((D + 3) // 4) * ((H + 7) // 8) * ((W + 7) // 8)
    return case.n * D * pick_strips(H)[0]


def pick_strips(H):
    """conv3d_row.hip pick_strips, restated -> (strips, rows per strip)"""
    for k in range(1, 9):
        if H % k == 0 and (H // k) % 4 == 0 and H // k <= 64:
            return k, H // k
    return 1, H


# ---- device side -------------------------------------------------------------------------------------------------------
SEEN = {}


def _bits(y):
    with np.errstate(over='ignore'):
        return (np.asarray(y, np.float64) + 0.0).astype(np.float16).view(np.uint16)


def _same_bits(got, want, what):
    g, w = _bits(got), _bits(want)
    if not np.array_equal(g, w):
        bad = np.argwhere(g != w)
        i = tuple(bad[0])
        raise AssertionError(f'{what}: {len(bad)} of {g.size} values differ, first at {i}: device {float(np.asarray(got)[i])!r} '
                             f'({g[i]:#06x}), reference {float(np.asarray(want)[i])!r} ({w[i]:#06x})')


def _knobs(case, monkeypatch):
    for name in KNOBS:
        monkeypatch.delenv(name, raising=False)
    for name, v in case.knobs.items():
        monkeypatch.setenv(name, v)


def _ran(case):
    from fast_nnunet_amd import capi
    ran = capi.op_last_kernels()
    assert ran == list(case.kernels), f'{case.id}: ran {ran}, the case is written for {list(case.kernels)}'
    SEEN.setdefault(case.id, set()).update(ran)


def _check_stats(stats, y16, mode, what):
    if R.stats_fit_exact(y16):
        assert np.array_equal(stats, R.stats_exact(y16)), f'{what}: statistics'
    else:
        assert mode != 'stats', f'{what}: the case claims exact statistics'


STEM_RUNS = [(c.id, m, f) for c in STEM_CASES for m in c.modes for f in (c.flips if m == 'ident' else c.flips[:1])]
FUSED_RUNS = [(c.id, m, f) for c in FUSED_STEM_CASES + FUSED_TCONV_CASES for m in c.modes
              for f in (c.flips if m == c.modes[0] else c.flips[:1])]


def _id(v):
    return ''.join(str(i) for i in v) if isinstance(v, tuple) else str(v)


@pytest.mark.parametrize('cid,mode,flips', STEM_RUNS, ids=_id)
def test_stem_equals_the_exact_reference(cid, mode, flips, monkeypatch):
    """fnn_op_stem == stem_exact bit for bit, per item of a batch cut from a sentinel-filled volume at non-zero origins;
    the statistics are the integers of the rounded outputs wherever their sums of squares stay exact."""
    from fast_nnunet_amd import capi
    case = BY_ID[cid]
    d, y16 = stem_reference(cid, mode, flips)
    _knobs(case, monkeypatch)
    y, stats = capi.op_stem(d['vol'], d['origins'], case.dims, d['w'], d['bias'], flips, want_stats=True)
    _ran(case)
    what = f'{cid} [{mode}, flips {flips}]'
    _same_bits(y, y16, what)
    if mode == 'round':                                       # y == f16(x): the one-hot centre tap of channel co % C
        x = np.stack([R.stem_window(d['vol'], o, flips, case.dims) for o in d['origins']])
        _same_bits(y, R.h16(x[:, [co % case.c for co in range(case.cout)]]) + 0.0, what + ': f16(x)')
    _check_stats(stats, y16, mode, what)


@pytest.mark.parametrize('cid,mode,flips', FUSED_RUNS, ids=_id)
def test_fused_consumer_equals_the_exact_composition(cid, mode, flips, monkeypatch):
    """fnn_op_conv_fused == conv_exact(stage16(f16(stem_exact))) resp. conv_exact(concat(f16(tconv_exact(stage16(low))),
    stage16(skip))) bit for bit; the consumer's statistics wherever they stay exact."""
    from fast_nnunet_amd import capi
    case = BY_ID[cid]
    d, amb, y16 = fused_reference(cid, mode, flips)
    assert amb == 0
    _knobs(case, monkeypatch)
    if case.kind == 'fstem':
        y, stats = capi.op_conv_fused_stem(d['vol'], d['origins'], case.dims, d['sw'], d['sbias'], d['norm'], d['slope'], d['w'], d['bias'], flips)
    else:
        y, stats = capi.op_conv_fused_tconv(d['low'], d['lnorm'], d['lslope'], d['tw'], d['tbias'], case.tstride, d['skip'], d['snorm'],
                                            d['sslope'], d['w'], d['bias'])
    _ran(case)
    what = f'{cid} [{mode}, flips {flips}]'
    _same_bits(y, y16, what)
    _check_stats(stats, y16, mode, what)


def test_fused_op_refuses_what_conv_choose_refuses(monkeypatch):
    """FNN_E_UNSUPPORTED (NotImplementedError), not another kernel: a transposed conv of two stride phases, a (3, 1, 3) pair"""
    from fast_nnunet_amd import capi
    for name in KNOBS:
        monkeypatch.delenv(name, raising=False)
    z = lambda *shape: np.zeros(shape, np.float32)
    with pytest.raises(NotImplementedError):
        capi.op_conv_fused_tconv(z(1, 32, 3, 8, 8), None, 1.0, z(32, 16, 1, 1, 2), None, (1, 1, 2), z(1, 16, 3, 8, 16), None, 1.0,
                                 z(16, 32, 1, 3, 3), None)
    vol, org = place(z(1, 1, 3, 8, 16), own=False)
    with pytest.raises(NotImplementedError):
        capi.op_conv_fused_stem(vol, org, (3, 8, 16), z(16, 1, 3, 1, 3), None, (np.ones(16), np.zeros(16)), SLOPE, z(16, 16, 3, 1, 3), None)


def test_every_stem_and_fused_kernel_form_is_asserted_by_a_case():
    """The closing test: every form of the family is an asserted kernel of a committed case, and whatever ran in this
    session ran what its case names (after a full run of this file: all of them)."""
    named = set().union(*(c.kernels for c in CASES))
    assert REQUIRED_KERNELS <= named, sorted(REQUIRED_KERNELS - named)
    ran = set().union(*SEEN.values()) if SEEN else set()
    assert ran <= named
    if all(c.id in SEEN for c in CASES):
        assert REQUIRED_KERNELS <= ran, sorted(REQUIRED_KERNELS - ran)
