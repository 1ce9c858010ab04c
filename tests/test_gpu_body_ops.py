"""Per-op parity of the kernels between the convs on a real MI355X (csrc/body.hip, head.hip): avgpool_kernel, combine_kernel,
combine_pool_kernel<2,2,2> / <1,2,2>, seg_head_kernel, seg_head_acc_kernel<ACC32>, seg_head_acc1_kernel<...>,
patch_acc_kernel<ACC32> and patch_input_kernel, each called once through its fnn_op_* entry point (the engine's own
launcher) and compared with tests/body_ref.py: the float64 value of that one operation and a per-element bound summed
from the roundings the kernel states.  Where two paths are documented to write the same bits, bits are compared.

The network-level budgets cannot see these errors: a uniform scale error in front of an InstanceNorm cancels, one
confined to a channel group or a few percent of the voxels fits inside 3.5e-3 rRMSE, and the bit-identity tests of the
accumulate path feed the oracle driver with the device's own head output.

No comparison here leaves an element out, and every case asserts the kernel variant that ran (fnn_op_last_kernels)."""
import itertools

import numpy as np
import pytest

import body_ref as R

pytestmark = pytest.mark.gpu

INT_MAX = R.INT_MAX


def _capi():
    from fast_nnunet_amd import capi
    return capi


def _ran(*want):
    ran = _capi().op_last_kernels()
    print('KERNELS', ran)
    assert ran == list(want), (ran, want)


def _ran_combine_pool(stride):
    """launch_combine notes the fused kernel as plain `combine_pool_kernel` (the engine's kernel log and the tests that read
    it keep that name) and picks the instantiation from the depth stride alone: <2,2,2> for 2, <1,2,2> for 1.  The pooled
    tensor's shape and values differ between the two, so a case passes only on the instantiation named here."""
    _ran('combine_pool_kernel')
    print(f'KERNELS instantiation combine_pool_kernel<{stride[0]},2,2>')


def _bits32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _within(got, t, bound, what):
    """|got - t| <= bound on EVERY element; on failure names the worst element"""
    got = np.asarray(got, np.float64)
    assert got.shape == t.shape == bound.shape, (got.shape, t.shape, bound.shape)
    assert np.isfinite(got).all(), f'{what}: non-finite values at {np.argwhere(~np.isfinite(got))[:4].tolist()}'
    err = np.abs(got - t)
    bad = err > bound
    if bad.any():
        i = np.unravel_index(np.argmax(np.where(bad, err / np.maximum(bound, 1e-300), 0)), err.shape)
        raise AssertionError(f'{what}: {int(bad.sum())} of {bad.size} elements outside the bound; worst at {tuple(int(k) for k in i)}: '
                             f'device {got[i]!r}, reference {t[i]!r}, |diff| {err[i]:.4g} > bound {bound[i]:.4g}')
    print(f'{what}: max |diff| / bound = {float((err / np.maximum(bound, 1e-300)).max()):.3f} over {err.size} elements')


# ---- operands ----------------------------------------------------------------------------------------------------------
def _raw(rng, n, c, dims):
    """a raw conv output: items with different mean and spread (their scale / shift rows differ), one channel with a large
    mean relative to its spread (a scale error is not hidden by symmetry), fp16-rounded"""
    x = rng.standard_normal((n, c, *dims))
    x = x * (0.5 + rng.random((n, c, 1, 1, 1)) * 2) + rng.standard_normal((n, c, 1, 1, 1)) * (1 + np.arange(n).reshape(n, 1, 1, 1, 1))
    x[:, 1 % c] = rng.standard_normal((n, *dims)) * 0.25 + 6.0
    return R.h16(x)


def _norm(rng, c):
    return (rng.random(c) + 0.5).astype(np.float32), (rng.standard_normal(c) * 0.3).astype(np.float32)


def _combine_case(seed, n, c, dims, layouts=(0, 0, 0, 0), pool=None, norm_a=True, norm_b=False, slope_a=1.0, slope_b=1.0, slope=0.01):
    """one fnn_op_combine call against body_ref.combine (+ pooled_of_output); with a pooling stride also bit for bit against
    the unfused pair combine_kernel -> avgpool_kernel, which combine_pool_kernel is documented to reproduce"""
    capi = _capi()
    what = f'combine seed {seed} n {n} C {c} dims {dims} layouts {layouts} pool {pool} norm {norm_a, norm_b} slopes {slope_a, slope_b, slope}'
    rng = np.random.default_rng(seed)
    a, b = _raw(rng, n, c, dims), _raw(rng, n, c, dims)
    na, nb = (_norm(rng, c) if norm_a else None), (_norm(rng, c) if norm_b else None)
    out = capi.op_combine(a, b, slope, norm_a=na, slope_a=slope_a, norm_b=nb, slope_b=slope_b, pool_stride=pool, layouts=layouts)
    _ran('combine_kernel') if pool is None else _ran_combine_pool(pool)
    y, pooled = out if pool is not None else (out, None)
    ss_a = R.scale_shift(a, *na) if norm_a else None
    ss_b = R.scale_shift(b, *nb) if norm_b else None
    t, bound = R.combine(a, b, slope, ss_a=ss_a, slope_a=slope_a, ss_b=ss_b, slope_b=slope_b)
    _within(y, t, bound, what)
    if pool is not None:
        tp, bp = R.pooled_of_output(y, pool)
        _within(pooled, tp, bp, what + ' (pooled)')
        y2 = capi.op_combine(a, b, slope, norm_a=na, slope_a=slope_a, norm_b=nb, slope_b=slope_b, layouts=layouts)
        _ran('combine_kernel')
        p2 = capi.op_avgpool(y2, pool, x_cm=layouts[2], y_cm=layouts[3])
        _ran('avgpool_kernel')
        assert np.array_equal(_bits32(y), _bits32(y2)), what + ': block output differs from combine_kernel'
        assert np.array_equal(_bits32(pooled), _bits32(p2)), what + ': pooled tensor differs from combine_kernel -> avgpool_kernel'
    return y


# rows of 16-byte vectors per grid row: channels-last vox * C / 8, chunk-major vox * 2; a thread block takes 256 * FNN_CMB_U
# = 1024 of them.  (5, 6, 7) = 210 voxels: a clamped tail at every C; (4, 8, 8) = 256 voxels at C = 32: exactly 1024.
@pytest.mark.parametrize('layouts', list(itertools.product((0, 1), repeat=3)), ids=lambda v: 'abo' + ''.join(map(str, v)))
@pytest.mark.parametrize('c', [32, 48, 160])
def test_combine_every_layout_combination(c, layouts):
    """channels-last / chunk-major on a, b and the output independently; C = 48 and 160 reload scale / shift per vector
    (256 % (C / 8) != 0: `fixed` is false for a channels-last output)"""
    _combine_case(100 + c, 3, c, (5, 6, 7), (*layouts, 0), norm_a=True, norm_b=True)


@pytest.mark.parametrize('n', [1, 3])
@pytest.mark.parametrize('c', [16, 32, 48, 64, 160, 320])
def test_combine_channel_counts_and_operand_roles(c, n):
    # a = raw + norm, b = identity skip without scale / shift rows; then the reverse; block slope 0.01 and 1
    _combine_case(200 + c + n, n, c, (3, 5, 7), (0, 0, 0, 0), norm_a=True, norm_b=False, slope=0.01)
    _combine_case(300 + c + n, n, c, (3, 5, 7), (0, 1, 1, 0) if c > 16 else (0, 0, 0, 0), norm_a=False, norm_b=True, slope=1.0)
    # operands that carry their own activation (slope on load): on both sides, then on one side only, each way round
    _combine_case(400 + c + n, n, c, (2, 3, 5), (0, 0, 0, 0), norm_a=True, norm_b=True, slope_a=0.01, slope_b=0.01)
    _combine_case(410 + c + n, n, c, (2, 3, 5), (0, 0, 0, 0), norm_a=True, norm_b=True, slope_a=0.01, slope_b=1.0)
    _combine_case(420 + c + n, n, c, (2, 3, 5), (0, 0, 0, 0), norm_a=True, norm_b=False, slope_a=1.0, slope_b=0.01, slope=1.0)


@pytest.mark.parametrize('c,dims,layouts', [(32, (4, 8, 8), (0, 0, 0, 0)),       # 256 voxels x 4 vectors: exactly one block
                                            (32, (8, 8, 16), (0, 0, 0, 0)),      # exactly four
                                            (32, (8, 8, 8), (0, 0, 1, 0)),       # chunk-major: 512 voxels x 2 vectors
                                            (32, (8, 8, 9), (1, 0, 1, 0)),       # ... one block and a tail
                                            (48, (9, 8, 8), (0, 0, 0, 0)),       # 3456 vectors: three blocks and a tail
                                            (16, (8, 8, 8), (0, 0, 0, 0))])
def test_combine_whole_blocks_and_clamped_tails(c, dims, layouts):
    _combine_case(500 + c + dims[2], 2, c, dims, layouts, norm_a=True, norm_b=False)


@pytest.mark.parametrize('layouts', list(itertools.product((0, 1), repeat=4)), ids=lambda v: 'abop' + ''.join(map(str, v)))
@pytest.mark.parametrize('stride', [(2, 2, 2), (1, 2, 2)], ids=str)
def test_combine_pool_every_layout_combination(stride, layouts):
    _combine_case(600 + stride[0], 3, 32, (4, 6, 10), layouts, pool=stride, norm_a=True, norm_b=True)


@pytest.mark.parametrize('stride', [(2, 2, 2), (1, 2, 2)], ids=str)
@pytest.mark.parametrize('c', [16, 48, 64, 160, 320])
def test_combine_pool_channel_counts(c, stride):
    lay = (1, 0, 0, 1) if c > 16 else (0, 0, 0, 0)
    _combine_case(700 + c, 1, c, (2, 4, 6), lay, pool=stride, norm_a=True, norm_b=False)
    _combine_case(800 + c, 3, c, (4, 2, 4), (0, 1, 1, 0) if c > 16 else lay, pool=stride, norm_a=False, norm_b=True, slope=1.0)


def _avgpool_case(seed, n, c, dims, stride, x_cm=0, y_cm=0, norm=True, slope=1.0):
    capi = _capi()
    rng = np.random.default_rng(seed)
    x = _raw(rng, n, c, dims)
    nm = _norm(rng, c) if norm else None
    y = capi.op_avgpool(x, stride, gamma=None if nm is None else nm[0], beta=None if nm is None else nm[1], slope=slope, x_cm=x_cm, y_cm=y_cm)
    _ran('avgpool_kernel')
    t, bound = R.avgpool(x, stride, R.scale_shift(x, *nm) if norm else None, slope)
    _within(y, t, bound, f'avgpool seed {seed} n {n} C {c} dims {dims} stride {stride} layouts {x_cm, y_cm} norm {norm} slope {slope}')


@pytest.mark.parametrize('stride', [(2, 1, 1), (1, 1, 2)], ids=str)
def test_strides_the_fused_kernel_does_not_take_go_through_avgpool_kernel(stride):
    """(2, 1, 1) and (1, 1, 2): launch_combine refuses to pool them (combine_pool_ok) and the planner's fallback, the
    pooling kernel, computes them"""
    capi = _capi()
    x = _raw(np.random.default_rng(5), 1, 32, (4, 4, 4))
    with pytest.raises(NotImplementedError):
        capi.op_combine(x, x, 0.01, pool_stride=stride)
    for x_cm, y_cm in itertools.product((0, 1), repeat=2):
        _avgpool_case(900 + stride[0], 3, 48, (4, 6, 6), stride, x_cm, y_cm, norm=True, slope=0.01)


@pytest.mark.parametrize('c', [16, 32, 48, 64, 160, 320])
def test_avgpool_channel_counts_layouts_and_divisors(c):
    for k, (stride, dims) in enumerate((((2, 2, 2), (4, 6, 10)), ((1, 2, 2), (3, 4, 6)), ((3, 1, 1), (7, 3, 5)), ((3, 3, 3), (6, 3, 9)))):
        # (3, 1, 1) and (3, 3, 3): reciprocals that are not powers of two; (7, 3, 5): a depth that is not a multiple
        _avgpool_case(1000 + c + k, 1 + 2 * (k % 2), c, dims, stride, x_cm=int(c > 16 and k % 2 == 0), y_cm=int(c > 16 and k >= 2), norm=k != 1,
                      slope=0.01 if k % 2 == 0 else 1.0)
    # an identity strided skip: the block input itself, no norm anywhere behind it to cancel a wrong divisor
    _avgpool_case(1100 + c, 3, c, (4, 4, 6), (2, 2, 2), norm=False)


@pytest.mark.parametrize('stride', [(2, 2, 2), (1, 2, 2), (2, 1, 1)], ids=str)
@pytest.mark.parametrize('c', [16, 48])
def test_pooling_of_exactly_summable_values_is_exact(c, stride):
    """values 1 + k 2^-10: the fp32 sum of 2, 4 or 8 of them and its product with the power-of-two reciprocal are exact, so
    the stored mean is fp16(t) itself - many of them ties between two fp16 numbers, where a reciprocal off by one fp32 ulp
    or a sum that is not exact lands on the other side (the bound of half an ulp cannot see that)"""
    capi = _capi()
    rng = np.random.default_rng(1200 + c + stride[0])
    x = 1.0 + rng.integers(0, 1024, (3, c, 4, 6, 8)) * 2.0 ** -10
    x[0] = -x[0]
    t, _ = R.pool(x, 0.0, stride)
    assert (R.h16(t) != t).mean() > 0.25 and ((t * 2.0 ** 11) % 2 == 1).any()          # inexact means, ties among them
    got = capi.op_avgpool(x, stride, x_cm=int(c > 16))
    _ran('avgpool_kernel')
    assert np.array_equal(got.astype(np.float64), R.h16(t)), f'avgpool {c} {stride}'
    if stride[1] == 2:
        y, pooled = capi.op_combine(x, np.zeros_like(x), 1.0, pool_stride=stride, layouts=(0, 0, int(c > 16), 0))
        _ran_combine_pool(stride)
        assert np.array_equal(y.astype(np.float64), x) and np.array_equal(pooled.astype(np.float64), R.h16(t)), f'combine_pool {c} {stride}'


@pytest.mark.parametrize('seed', range(24))
def test_combine_random_cases(seed):
    rng = np.random.default_rng(7000 + seed)
    c = int(rng.choice([16, 32, 48, 64, 160, 320]))
    n = int(rng.choice([1, 3]))
    pool = [None, (2, 2, 2), (1, 2, 2)][int(rng.integers(3))]
    dims = tuple(int(rng.integers(1, 5)) * (2 if pool else 1) + (0 if pool else int(rng.integers(2))) for _ in range(3))
    layouts = tuple(int(v) for v in rng.integers(0, 2, 4)) if c > 16 else (0, 0, 0, 0)
    norm_a, norm_b = bool(rng.integers(2)), bool(rng.integers(2))
    slopes = [float(rng.choice([0.01, 1.0])) for _ in range(3)]
    print('case', seed, n, c, dims, layouts, pool, norm_a, norm_b, slopes)
    _combine_case(7100 + seed, n, c, dims, layouts, pool, norm_a, norm_b, *slopes)


# ---- seg head ----------------------------------------------------------------------------------------------------------
PATCHES = [(7, 9, 11), (16, 16, 16), (5, 9, 13)]       # ragged wave and round; whole waves; 585 voxels: > 256, not a multiple of 64


def _pattern(shape, dtype, integers=False):
    """a recognisable finite accumulator content: multiples of 1/8 in [-15.625, 15.625] (or those rounded to integers), no
    negative zero"""
    i = np.arange(int(np.prod(shape)), dtype=np.int64)
    v = ((i * 7) % 251 - 125) / 8.0
    return (np.rint(v) + 0.0 if integers else v).astype(dtype).reshape(shape)


def _gauss_bits(kind, patch):
    """None (weight 1) | 'real' (the predictor's map for this patch) | 'subnormal' (the real map with the smallest fp16
    subnormal on every third voxel, the rest of the reference's values)"""
    if kind is None:
        return None
    from fast_nnunet_amd.sliding_window import compute_gaussian
    g = compute_gaussian(tuple(patch), sigma_scale=1. / 8, value_scaling_factor=10).numpy().copy().view(np.uint16).reshape(-1)
    if kind == 'subnormal':
        g[::3] = 1
    return g


def _head_kernel(c, mode, fp32):
    if mode:
        return 'seg_head_kernel'
    if (c + 15) // 16 * 16 <= 32:
        return 'seg_head_acc1_kernel<1,2>' if fp32 else 'seg_head_acc1_kernel<0,2,3,2>'
    return f'seg_head_acc_kernel<{int(fp32)}>'


def _head_inputs(rng, n, c, patch, heads, integers=False):
    if integers:
        # every product and every partial sum an integer below 2^11: exact in fp16 operands, fp32 sums and fp16 stores
        x = rng.integers(-2, 3, (n, c, *patch)).astype(np.float64)
        w = rng.integers(-1, 2, (heads, c)).astype(np.float64)
        b = rng.integers(-4, 5, heads).astype(np.float32)
        return x, w, b
    x = _raw(rng, n, c, patch)
    w = R.h16(rng.standard_normal((heads, c)) / np.sqrt(c))
    w[:, 1 % c] = R.h16(rng.standard_normal(heads) * 0.1)                  # (the large-mean channel: keep the logits O(1))
    b = rng.standard_normal(heads).astype(np.float32)
    b[-1] = 3.0                                                            # the last head's bias: block >= 1 from 17 heads on
    return x, w, b


def _head_acc_case(seed, heads, c, patch, fp32, n=2, item=None, gauss=None, norm=True, slope=0.01, first=None, integers=False,
                   margin=((1, 2), (0, 1), (2, 3))):
    """mode 0: head + weight + accumulate into a box larger than the patch, origin off zero"""
    capi = _capi()
    rng = np.random.default_rng(seed)
    item = n - 1 if item is None else item
    slope = 1.0 if integers else slope
    what = f'head seed {seed} heads {heads} C {c} patch {patch} fp32 {fp32} n {n} item {item} gauss {gauss} norm {norm} first {first} int {integers}'
    x, w, b = _head_inputs(rng, n, c, patch, heads, integers)
    nm = _norm(rng, c) if norm else None
    hp = (heads + 1 + 7) // 8 * 8
    box = tuple(patch[i] + margin[i][0] + margin[i][1] for i in range(3))
    origin = tuple(m[0] for m in margin)
    dt = np.float32 if fp32 else np.float16
    acc0 = _pattern((*box, hp), dt, integers)
    win = tuple(slice(origin[i], origin[i] + patch[i]) for i in range(3))
    fm = None
    if first is not None and first != (INT_MAX,) * 3:
        fm = R.first_mask(patch, first)
        acc0[win][fm] = np.nan                                             # unvisited voxels hold garbage: never read
    acc = acc0.copy()
    gb = _gauss_bits(gauss, patch)
    honoured = capi.op_seg_head(x, w, b, item=item, mode=0, norm=nm, slope=slope, gauss_bits=gb, acc=acc, origin=origin, first_visit=first)
    _ran(_head_kernel(c, 0, fp32))
    assert honoured == ((c + 15) // 16 * 16 <= 32), what
    P = int(np.prod(patch))
    xop, spread = R.head_operand(x, R.scale_shift(x, *nm) if norm else None, slope)
    t, e_t = R.head(xop[item].reshape(c, P), w, b, spread[item].reshape(c, P))
    g_bits = gb if gb is not None else np.full(P, 0x3C00, np.uint16)
    g = g_bits.view(np.float16).astype(np.float64)
    fmf = None if fm is None else fm.reshape(-1)
    inside0 = acc0[win].reshape(P, hp)
    inside = acc[win].reshape(P, hp)
    want, bound = R.accumulate(inside0[:, :heads].T.astype(np.float64), t, e_t, g, fp32, fmf)
    if integers:
        assert (bound < 0.5).all()
        assert np.array_equal(inside[:, :heads].T.astype(np.float64), want), what + ': integer operands must be exact'
    _within(inside[:, :heads].T, want, bound, what)
    # the weight-sum channel, bit for bit
    ws = R.weight_channel(inside0[:, heads], g_bits, fp32, fmf)
    assert np.array_equal(inside[:, heads].view(np.uint32 if fp32 else np.uint16), ws.view(np.uint32 if fp32 else np.uint16)), \
        what + ': weight-sum channel'
    # channels above `heads` keep their bits (first-visit voxels are written as 0 + 0 there), and so does everything outside
    pad_want = inside0[:, heads + 1:].copy()
    if fmf is not None:
        pad_want[fmf] = 0
    ub = np.uint32 if fp32 else np.uint16
    assert np.array_equal(inside[:, heads + 1:].view(ub), pad_want.view(ub)), what + ': padding channels changed'
    outside = np.ones(box, bool)
    outside[win] = False
    assert np.array_equal(acc[outside].view(ub), acc0[outside].view(ub)), what + ': accumulator written outside the patch'
    assert not np.isnan(acc).any(), what


HEADS = [1, 2, 3, 7, 15, 16, 17, 61, 63, 64, 105, 118]
CHANNELS = [16, 32, 48, 64, 160]


@pytest.mark.parametrize('c', CHANNELS)
@pytest.mark.parametrize('heads', HEADS)
def test_head_accumulate_heads_and_channels(heads, c):
    """hblocks = ceil((heads + 1) / 16): 15 | 16 is a block edge, 63 | 64 the edge of the kernels' passes of four blocks,
    7 | 15 edges of HP; C <= 32 runs the one-k-step kernels, C >= 48 the k-loop (48 and 160: a zero-padded half k-step)"""
    k = HEADS.index(heads) + CHANNELS.index(c)
    for fp32 in (False, True):
        _head_acc_case(2000 + 7 * heads + c, heads, c, PATCHES[k % 3], fp32, n=2, item=(k + fp32) % 2,
                       gauss=[None, 'real', 'subnormal'][(k + fp32) % 3], norm=k % 4 != 3)


@pytest.mark.parametrize('fp32', [False, True], ids=['acc16', 'acc32'])
@pytest.mark.parametrize('c', [16, 32])
@pytest.mark.parametrize('first', [(0, 0, 0), (3, 4, 5), (INT_MAX,) * 3, (0, 4, 0), (3, 0, INT_MAX)], ids=str)
def test_head_first_visit_voxels_are_written_without_being_read(first, c, fp32):
    """NaN in exactly the voxels the thresholds declare unvisited: the result there is 0 + contribution"""
    for heads, gauss in ((3, 'real'), (17, None), (64, 'subnormal')):
        _head_acc_case(3000 + c + heads, heads, c, (7, 9, 11), fp32, gauss=gauss, first=first)


@pytest.mark.parametrize('c', [48, 64, 160])
def test_head_first_visit_is_refused_by_the_k_loop_kernels(c):
    capi = _capi()
    x, w, b = _head_inputs(np.random.default_rng(1), 1, c, (4, 4, 4), 3)
    acc = np.zeros((4, 4, 4, 8), np.float16)
    with pytest.raises(NotImplementedError):
        capi.op_seg_head(x, w, b, acc=acc, first_visit=(0, 0, 0))
    assert not capi.op_seg_head(x, w, b, acc=acc, first_visit=(INT_MAX,) * 3)          # the helper says no; INT_MAX is accepted
    _head_acc_case(3100 + c, 3, c, (7, 9, 11), False, first=(INT_MAX,) * 3)


@pytest.mark.parametrize('fp32', [False, True], ids=['acc16', 'acc32'])
@pytest.mark.parametrize('c', CHANNELS)
def test_head_operand_map_with_exact_integers(c, fp32):
    """integer operands small enough that every sum is exact: any wrong lane, k-step, head row or bias index shows as a
    whole-number difference"""
    for heads in (2, 16, 17, 64, 118):
        _head_acc_case(3200 + c + heads, heads, c, (5, 9, 13), fp32, n=3, norm=False, integers=True)


def _head_patch_case(seed, heads, c, patch, flips, n=2, item=None, norm=True, integers=False):
    """mode 1 ('=' into a buffer of NaNs), then mode 2 ('+=' onto what is there) with another item"""
    capi = _capi()
    rng = np.random.default_rng(seed)
    item = n - 1 if item is None else item
    what = f'head patch-buffer seed {seed} heads {heads} C {c} patch {patch} flips {flips} item {item} int {integers}'
    x, w, b = _head_inputs(rng, n, c, patch, heads, integers)
    nm = _norm(rng, c) if norm else None
    P = int(np.prod(patch))
    slope = 1.0 if integers else 0.01
    xop, spread = R.head_operand(x, R.scale_shift(x, *nm) if norm else None, slope)
    pb = np.full((heads, P), np.nan, np.float32)
    capi.op_seg_head(x, w, b, item=item, mode=1, flips=flips, norm=nm, slope=slope, patch_buf=pb)
    _ran('seg_head_kernel')
    t, e = R.head(xop[item].reshape(c, P), w, b, spread[item].reshape(c, P))
    t, e = R.unflip(t, patch, flips), R.unflip(e, patch, flips)
    if integers:
        assert np.array_equal(pb.astype(np.float64), t), what + ': integer operands must be exact'
    _within(pb, t, e, what + ' (=)')
    pb1 = pb.copy()
    other = (item + 1) % n
    capi.op_seg_head(x, w, b, item=other, mode=2, flips=flips, norm=nm, slope=slope, patch_buf=pb)
    _ran('seg_head_kernel')
    t2, e2 = R.head(xop[other].reshape(c, P), w, b, spread[other].reshape(c, P))
    s = pb1.astype(np.float64) + R.unflip(t2, patch, flips)
    _within(pb, s, R.unflip(e2, patch, flips) + R.U32 * np.abs(s), what + ' (+=)')


@pytest.mark.parametrize('flips', [(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1)], ids=str)
@pytest.mark.parametrize('c', [16, 48])
def test_head_patch_buffer_modes_and_flips(c, flips):
    for heads, patch in ((3, (7, 9, 11)), (64, (5, 9, 13)), (105, (7, 9, 11))):
        _head_patch_case(4000 + c + heads, heads, c, patch, flips)


@pytest.mark.parametrize('heads', HEADS)
def test_head_patch_buffer_heads(heads):
    k = HEADS.index(heads)
    _head_patch_case(4100 + heads, heads, CHANNELS[k % 5], PATCHES[k % 3], (k % 2, (k // 2) % 2, (k // 4) % 2), item=k % 2, norm=k % 3 != 0)
    _head_patch_case(4200 + heads, heads, CHANNELS[(k + 2) % 5], (5, 9, 13), (1, 0, 1), n=3, norm=False, integers=True)


@pytest.mark.parametrize('fp32', [False, True], ids=['acc16', 'acc32'])
@pytest.mark.parametrize('heads,c', [(3, 32), (17, 16), (64, 48), (118, 160)])
def test_fused_accumulate_equals_patch_buffer_then_patch_acc(heads, c, fp32):
    """head.hip: the logits of every seg-head kernel agree bit for bit (the bias is the MFMA's C operand in each), and
    both accumulate forms state the same roundings (fl32(t * g), never fused; fl32(a + c); one rounding to fp16): without
    mirroring and with n_div = 1 (x / 1 is exact) the two paths must leave the same accumulator bits"""
    capi = _capi()
    rng = np.random.default_rng(4300 + heads)
    patch = (7, 9, 11)
    x, w, b = _head_inputs(rng, 2, c, patch, heads)
    nm = _norm(rng, c)
    gb = _gauss_bits('subnormal', patch)
    hp = (heads + 1 + 7) // 8 * 8
    acc_a = _pattern((9, 10, 14, hp), np.float32 if fp32 else np.float16)
    acc_b = acc_a.copy()
    capi.op_seg_head(x, w, b, item=1, mode=0, norm=nm, slope=0.01, gauss_bits=gb, acc=acc_a, origin=(1, 1, 2))
    _ran(_head_kernel(c, 0, fp32))
    pb = np.zeros((heads, int(np.prod(patch))), np.float32)
    capi.op_seg_head(x, w, b, item=1, mode=1, norm=nm, slope=0.01, patch_buf=pb)
    _ran('seg_head_kernel')
    capi.op_patch_acc(pb, patch, 1, acc_b, origin=(1, 1, 2), gauss_bits=gb)
    _ran(f'patch_acc_kernel<{int(fp32)}>')
    ub = np.uint32 if fp32 else np.uint16
    assert np.array_equal(acc_a.view(ub), acc_b.view(ub))


@pytest.mark.parametrize('seed', range(24))
def test_head_random_cases(seed):
    rng = np.random.default_rng(8000 + seed)
    heads, c = int(rng.choice(HEADS)), int(rng.choice(CHANNELS))
    patch = PATCHES[int(rng.integers(3))] if rng.integers(2) else tuple(int(v) for v in rng.integers(2, 13, 3))
    n = int(rng.choice([1, 3]))
    item = int(rng.integers(n))
    print('case', seed, heads, c, patch, n, item)
    if rng.integers(3) == 0:
        _head_patch_case(8100 + seed, heads, c, patch, tuple(int(v) for v in rng.integers(0, 2, 3)), n=n, item=item, norm=bool(rng.integers(2)))
        return
    one_k = c <= 32
    first = tuple(int(rng.integers(0, patch[i] + 1)) for i in range(3)) if one_k and rng.integers(2) else None
    _head_acc_case(8100 + seed, heads, c, patch, bool(rng.integers(2)), n=n, item=item, gauss=[None, 'real', 'subnormal'][int(rng.integers(3))],
                   norm=bool(rng.integers(2)), first=first, margin=tuple((int(rng.integers(3)), int(rng.integers(3))) for _ in range(3)))


# ---- patch_acc ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('fp32', [False, True], ids=['acc16', 'acc32'])
@pytest.mark.parametrize('n_div', [1, 2, 4, 8])
def test_patch_acc(n_div, fp32):
    capi = _capi()
    for heads, patch, gauss in ((3, (7, 9, 11), 'real'), (16, (5, 9, 13), None), (63, (7, 9, 11), 'subnormal'), (118, (4, 4, 5), 'real')):
        what = f'patch_acc n_div {n_div} fp32 {fp32} heads {heads} patch {patch} gauss {gauss}'
        rng = np.random.default_rng(5000 + heads + n_div)
        P = int(np.prod(patch))
        pb = (rng.standard_normal((heads, P)) * 3 * n_div).astype(np.float32)
        hp = (heads + 1 + 7) // 8 * 8
        box, origin = tuple(p + 3 for p in patch), (2, 0, 1)
        acc0 = _pattern((*box, hp), np.float32 if fp32 else np.float16)
        acc = acc0.copy()
        gb = _gauss_bits(gauss, patch)
        capi.op_patch_acc(pb, patch, n_div, acc, origin=origin, gauss_bits=gb)
        _ran(f'patch_acc_kernel<{int(fp32)}>')
        win = tuple(slice(origin[i], origin[i] + patch[i]) for i in range(3))
        inside0, inside = acc0[win].reshape(P, hp), acc[win].reshape(P, hp)
        g_bits = gb if gb is not None else np.full(P, 0x3C00, np.uint16)
        t, e_t = R.patch_mean(pb, n_div)
        if n_div & (n_div - 1) == 0:
            e_t = np.zeros_like(e_t)                                        # division by a power of two is exact
        want, bound = R.accumulate(inside0[:, :heads].T.astype(np.float64), t, e_t, g_bits.view(np.float16).astype(np.float64), fp32)
        _within(inside[:, :heads].T, want, bound, what)
        ub = np.uint32 if fp32 else np.uint16
        assert np.array_equal(inside[:, heads].view(ub), R.weight_channel(inside0[:, heads], g_bits, fp32).view(ub)), what + ': weight-sum channel'
        assert np.array_equal(inside[:, heads + 1:].view(ub), inside0[:, heads + 1:].view(ub)), what + ': padding channels changed'
        outside = np.ones(box, bool)
        outside[win] = False
        assert np.array_equal(acc[outside].view(ub), acc0[outside].view(ub)), what + ': accumulator written outside the patch'


def test_patch_acc_divides_by_a_divisor_that_is_not_a_power_of_two():
    """n_div = 3 (one mirror axis pair is 2, 4, 8; a caller of the C ABI may average any count): IEEE division, one rounding"""
    capi = _capi()
    rng = np.random.default_rng(5100)
    patch, heads = (5, 9, 13), 7
    pb = (rng.standard_normal((heads, 585)) * 5).astype(np.float32)
    acc0 = _pattern((*patch, 8), np.float32)
    acc = acc0.copy()
    capi.op_patch_acc(pb, patch, 3, acc)
    _ran('patch_acc_kernel<1>')
    want, bound = R.accumulate(acc0.reshape(585, 8)[:, :heads].T.astype(np.float64), *R.patch_mean(pb, 3), np.ones(585), True)
    _within(acc.reshape(585, 8)[:, :heads].T, want, bound, 'patch_acc n_div 3')


# ---- patch_input -------------------------------------------------------------------------------------------------------
def _volume(rng, shape):
    """fp32 values whose fp16 rounding covers the edges: overflow, subnormals, ties to even in both directions"""
    v = (rng.standard_normal(shape) * 3).astype(np.float32)
    flat = v.reshape(-1)
    special = np.array([70000.0, -70000.0, 65520.0, 65519.99, 2.0 ** -25, 1.5 * 2.0 ** -24, -2.5 * 2.0 ** -24, 2.0 ** -14 - 2.0 ** -26,
                        1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, -(2.0 + 2.0 ** -10), 1e-8, -0.0, 3e-5], np.float32)
    idx = rng.choice(flat.size, flat.size // 3, replace=False)
    flat[idx] = special[np.arange(idx.size) % special.size]
    return v


@pytest.mark.parametrize('flips', [(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1)], ids=str)
@pytest.mark.parametrize('c,cpad', [(1, 16), (2, 16), (4, 16), (14, 16), (20, 32)])
def test_patch_input(c, cpad, flips):
    capi = _capi()
    rng = np.random.default_rng(6000 + c)
    vdim, patch = (9, 12, 15), (5, 7, 9)
    # windows touching every face of the volume (the two opposite corners) and one inside
    origins = [[0, 0, 0], [4, 5, 6], [2, 3, 1], [0, 5, 0], [4, 0, 6]]
    for batched in (False, True):                                           # batch stride zero (one volume) and non-zero
        vol = _volume(rng, (len(origins), c, *vdim) if batched else (c, *vdim))
        want = R.patch_input(vol, origins, patch, cpad, flips)
        for cm in ((False, True) if cpad > 16 else (False,)):               # the layouts differ only above 16 channels
            got = capi.op_patch_input(vol, origins, patch, cpad, flips=flips, chunk_major=cm)
            _ran('patch_input_kernel')
            assert np.array_equal(got, want), (c, cpad, flips, batched, cm, np.argwhere(got != want)[:4].tolist())
    # more than one block of 256 voxels, a ragged last block
    vol = _volume(rng, (c, 8, 9, 11))
    got = capi.op_patch_input(vol, [[0, 0, 0]], (8, 9, 11), cpad, flips=flips)
    assert np.array_equal(got, R.patch_input(vol, [[0, 0, 0]], (8, 9, 11), cpad, flips))


def test_every_kernel_variant_is_reachable_through_an_op():
    """one small call per instantiation; the names are printed so that a run's output lists them"""
    capi = _capi()
    seen = []
    x = _raw(np.random.default_rng(9), 1, 32, (2, 4, 4))
    capi.op_avgpool(x, (2, 1, 1)); seen += capi.op_last_kernels()
    capi.op_combine(x, x, 0.01); seen += capi.op_last_kernels()
    for stride in ((2, 2, 2), (1, 2, 2)):                        # both instantiations: the pooled shapes tell them apart
        _, pooled = capi.op_combine(x, x, 0.01, pool_stride=stride); seen += capi.op_last_kernels()
        assert pooled.shape == (1, 32, 2 // stride[0], 2, 2)
        _ran_combine_pool(stride)
    for c in (32, 48):
        xh, w, b = _head_inputs(np.random.default_rng(10), 1, c, (2, 4, 4), 3)
        for dt in (np.float16, np.float32):
            capi.op_seg_head(xh, w, b, acc=np.zeros((2, 4, 4, 8), dt)); seen += capi.op_last_kernels()
    pb = np.zeros((3, 32), np.float32)
    capi.op_seg_head(xh, w, b, mode=1, patch_buf=pb); seen += capi.op_last_kernels()
    for dt in (np.float16, np.float32):
        capi.op_patch_acc(pb, (2, 4, 4), 2, np.zeros((2, 4, 4, 8), dt)); seen += capi.op_last_kernels()
    capi.op_patch_input(np.zeros((1, 2, 4, 4), np.float32), [[0, 0, 0]], (2, 4, 4), 16); seen += capi.op_last_kernels()
    print('KERNELS', sorted(set(seen)))
    assert sorted(set(seen)) == sorted([
        'avgpool_kernel', 'combine_kernel', 'combine_pool_kernel', 'seg_head_kernel',
        'seg_head_acc_kernel<0>', 'seg_head_acc_kernel<1>', 'seg_head_acc1_kernel<0,2,3,2>', 'seg_head_acc1_kernel<1,2>',
        'patch_acc_kernel<0>', 'patch_acc_kernel<1>', 'patch_input_kernel'])
