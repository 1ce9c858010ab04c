"""tests/conv_ref.py without a GPU: the restatement is the oracle's operation up to the fp16 roundings it states, its
one-rounding arithmetic is exact (checked against rational arithmetic), and EVERY case tests/test_gpu_conv_exact.py commits
is what it claims to be - unambiguous operands, exact sums, exact statistics - and discriminates: mutants of the reference
change the outputs of the case meant to catch them."""
import os
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import body_ref as B  # noqa: E402
import conv_ref as R  # noqa: E402
import test_gpu_conv_exact as G  # noqa: E402
from oracle.unet import ConvNormAct  # noqa: E402


# ---- the restatement against the oracle ----------------------------------------------------------------------------------
def test_stage16_and_conv_exact_are_the_oracles_conv_norm_act_up_to_the_stated_roundings():
    torch.manual_seed(3)
    a = ConvNormAct(5, 7, (3, 3, 3), (1, 1, 1), True, 1e-5, 0.01).double().eval()
    b = ConvNormAct(7, 6, (3, 3, 3), (2, 1, 2), True, 1e-5, 0.01).double().eval()
    with torch.no_grad():
        a.norm.weight.copy_(torch.rand(7) + 0.5)
        a.norm.bias.copy_(torch.randn(7) * 0.3)
        x = torch.randn(2, 5, 6, 9, 10, dtype=torch.float64)
        raw = torch.from_numpy(B.h16(a.conv(x).numpy()))                       # what the producer stored
        want = F.leaky_relu(a.norm(raw), 0.01).numpy()
    gamma, beta = a.norm.weight.detach().numpy(), a.norm.bias.detach().numpy()
    v, lo, hi, amb = R.stage16(raw.numpy(), (gamma, beta), 0.01)
    sc, sh, _, _ = B.scale_shift(raw.numpy(), gamma, beta, exact=True)
    ex = (slice(None), slice(None), None, None, None)
    mag = np.abs(raw.numpy() * sc[ex]) + np.abs(sh[ex])
    # f16(sc), f16(sh), the rounding of o, f16(slope) and the rounding of the slope product: half an fp16 ulp of each; the
    # wrapper's f32 count reciprocal and eps move (sc, sh) by parts in 1e7
    bound = 2.0 ** -11 * (mag + np.abs(want) * 3) + 1e-6 * mag + 2.0 ** -24
    assert (np.abs(v - want) <= bound).all(), (np.abs(v - want) / bound).max()
    assert amb == 0 and np.array_equal(lo, v) and np.array_equal(hi, v)
    w, bias = B.h16(b.conv.weight.detach().numpy()), b.conv.bias.detach().numpy().astype(np.float32)
    t, y16 = R.conv_exact(v, w, bias, (3, 3, 3), (2, 1, 2))
    with torch.no_grad():
        b.conv.weight.copy_(torch.from_numpy(w))
        b.conv.bias.copy_(torch.from_numpy(bias.astype(np.float64)))
        ref = b.conv(torch.from_numpy(v)).numpy()
    assert np.abs(t - ref).max() <= 1e-12 * np.abs(ref).max()
    assert np.array_equal(y16, B.h16(t) + 0.0)
    up = torch.nn.ConvTranspose3d(7, 4, (2, 1, 2), (2, 1, 2)).double()
    tt, _ = R.tconv_exact(v, up.weight.detach().numpy(), up.bias.detach().numpy().astype(np.float32), (2, 1, 2))
    with torch.no_grad():
        up.bias.copy_(torch.from_numpy(up.bias.detach().numpy().astype(np.float32).astype(np.float64)))
        assert np.abs(tt - up(torch.from_numpy(v)).numpy()).max() <= 1e-12 * np.abs(tt).max()


def _rn16(fr):
    """a Fraction rounded to the nearest fp16 (ties to even), exactly; magnitudes below fp16's overflow"""
    if fr == 0:
        return 0.0
    e = -14
    while Fraction(2) ** (e + 1) <= abs(fr):
        e += 1
    ulp = Fraction(2) ** (e - 10)
    q = fr / ulp
    n = q.numerator // q.denominator
    rem = q - n
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and n % 2):
        n += 1
    return float(n * ulp)


def test_one_rounding_arithmetic_against_rational_arithmetic():
    rs = np.random.RandomState(5)
    bits = rs.randint(0, 0x7800, 3 * 3000).astype(np.uint16) | (rs.randint(0, 2, 9000).astype(np.uint16) << 15)
    x, s, h = bits.view(np.float16).astype(np.float64).reshape(3, -1)
    keep = (np.abs(x * s) + np.abs(h) < 60000) & R.span_ok(x, s, h)
    assert keep.sum() > 1500
    # ties by construction: h with exponent e (ulp 2^(e - 10)), x an odd integer, s = 2^(e - 11): x s = (k + 1/2) ulp
    e = rs.randint(-12, 5, 1500)
    h_t = np.ldexp((1024 + rs.randint(0, 1024, 1500)).astype(np.float64), e - 10) * rs.choice([-1, 1], 1500)
    x_t = (2 * rs.randint(0, 60, 1500) + 1).astype(np.float64) * rs.choice([-1, 1], 1500)
    s_t = np.ldexp(1.0, e - 11)
    x, s, h = np.concatenate((x[keep], x_t)), np.concatenate((s[keep], s_t)), np.concatenate((h[keep], h_t))
    got = R.fma16(x, s, h)
    want = np.array([_rn16(Fraction(a) * Fraction(b) + Fraction(c)) for a, b, c in zip(x, s, h)])
    assert np.array_equal(got, want)
    exact = np.array([Fraction(a) * Fraction(b) + Fraction(c) for a, b, c in zip(x_t, s_t, h_t)])
    assert sum(1 for f, g in zip(exact, got[-1500:]) if f != Fraction(g)) > 1400        # the ties do round
    two = B.h16(B.h16(x * s) + h)
    assert (two != got).any()                                                             # ... and two roundings are visible
    o = got[np.abs(got) < 1000]
    want = np.array([max(Fraction(v), Fraction(_rn16(Fraction(v) * Fraction(float(np.float16(0.01)))))) for v in o])
    assert np.array_equal(R.act16(o, 0.01), want.astype(np.float64))


def test_quantum_and_the_exactness_predicates():
    assert R.quantum(np.array([6.0, 0.0, -10.0])) == 2.0 and R.quantum(np.array([0.75]), np.array([2.0])) == 0.25
    assert R.quantum(np.zeros(3)) == 1.0
    a, w = np.full((1, 2, 1, 1, 3), 3.0), np.full((4, 2, 1, 1, 3), 2.0)
    assert R.fits_exact(a, w, np.full(4, 0.5))
    assert not R.fits_exact(a * 2.0 ** 20, w, np.full(4, 0.5))                            # 2^24 quanta of 0.5 are exceeded
    assert R.stats_fit_exact(np.full((1, 1, 4095), 64.0)) and not R.stats_fit_exact(np.concatenate((np.full((1, 1, 4096), 64.0), np.ones((1, 1, 1))), 2))
    assert np.array_equal(R.stats_exact(np.array([[[1.0, -3.0]]])), [[[-2.0, 10.0]]])


def test_craft_norm_lands_on_its_fp16_targets():
    rs = np.random.RandomState(1)
    first = 2.0 * rs.randint(-4, 5, (8, 600))
    x = G._permuted_items(first, 3).reshape(3, 8, 5, 10, 12)
    S = np.array([R.F16_TARGETS[c % 4][0] for c in range(8)])
    H = np.array([R.F16_TARGETS[c % 4][1] for c in range(8)])
    gamma, beta = R.craft_norm(x, S, H)
    sc, sh, _, _ = B.scale_shift(x, gamma, beta)
    assert np.abs(sc / S - 1).max() <= 1.2e-7
    sc_h, sh_h, _, amb = R.stage_params(x, (gamma, beta), margin=4.0)
    assert amb == 0 and (sc_h == S).all() and (sh_h == H).all()
    v, _, _, _ = R.stage16(x, (gamma, beta), 0.25)
    o = x * S[None, :, None, None, None] + H[None, :, None, None, None]
    assert np.array_equal(v, np.maximum(o, o * 0.25))


# ---- every committed GPU case -------------------------------------------------------------------------------------------
def _runs():
    runs = [(c, m) for c in G.DENSE_CASES for m in c.modes]
    runs += [(G.BY_ID[i], m) for i in G.STORE_CASES for m in G.STORE_MODES]
    return runs + [(c, 'const') for c in G.CONST_CASES]


@pytest.mark.parametrize('case,mode', _runs(), ids=lambda v: v.id if isinstance(v, G.Case) else v)
def test_committed_case_is_unambiguous_and_exact(case, mode):
    d = G.case_data(case, mode)
    for x, norm in ((d['x'], d['norm']), (d['x2'], d['norm2'])):
        if norm is not None:
            assert R.stage_params(x, norm, margin=4.0)[3] == 0
    a, lo, hi, amb = G.case_staged(d)
    assert amb == 0 and lo is not None
    w = d['w'].swapaxes(0, 1) if case.kind == 'tconv' else d['w']
    if mode == 'const' and case.kernel.startswith(G.FP32_STAGING):
        # the fp32 form: a bracket per element (open on the near-constant channels, where 7 u of |x sc| reaches an fp16 ulp of the
        # result); the sums stay exact at both ends and it is another value than the fp16 form's on this data (a kernel on the
        # wrong form fails the case)
        v32, lo, hi, n_open = R.stage32(d['x'], d['norm'], d['slope'])
        assert (lo[:, :1] == hi[:, :1]).mean() > 0.99 and R.fits_exact(lo, w, None) and R.fits_exact(hi, w, None)
        assert ((a < lo) | (a > hi)).mean() > 0.3
        a = v32
    assert R.fits_exact(a, w, d['bias']), 'the sums of this case are not exact in fp32'
    if mode in ('norm', 'two'):
        sc_h, sh_h, _, _ = R.stage_params(d['x'], d['norm'])
        off = G.SRC_NORM[0][0]
        assert all(sc_h[0, c] == R.F16_TARGETS[(c + off) % 4][0] and sh_h[0, c] == R.F16_TARGETS[(c + off) % 4][1] for c in range(case.cin))
    if mode in G.STORE_MODES or mode in ('const', 'stats', 'statsround'):
        t, y16 = G.case_reference(case, d, a)
        if mode in ('stats', 'statsround'):
            assert R.stats_fit_exact(y16), 'the case claims exact statistics'
        if mode == 'statsround':                                   # the store rounds: sums of accumulators are other numbers
            assert (t != y16).mean() > 0.3 and not np.array_equal(R.stats_exact(t), R.stats_exact(y16))
        if mode == 'ties':
            frac, mag = np.abs(t) % 1.0, np.abs(t)
            assert ((frac == 0.5) & (mag > 1024) & (mag < 2048)).sum() >= 20 and (mag > 2048).sum() >= 20 and (t == 0).sum() >= 1
        if mode == 'subnormal':
            assert ((np.abs(t) < 2.0 ** -14) & (t != 0)).mean() > 0.5 and ((np.abs(t) / 2.0 ** -24) % 1.0 == 0.5).sum() >= 20


def test_persistent_cases_have_range_seams_inside_items():
    """a persistent workgroup walks total / workgroups tiles: with fewer items than workgroups that is less than an item's
    tiles, so ranges end inside items (the seam the issue asks the comparison to cover)"""
    seen = set()
    for c in G.DENSE_CASES:
        for name, wgs in G.PERSISTENT_WGS.items():
            if c.kernel.startswith(name):
                assert 1 < c.n < wgs, c.id
                seen.add(name)
    assert seen == set(G.PERSISTENT_WGS)


def test_row_over_grid_cases_walk_units_across_planes_and_items():
    """the row kernels' units are (plane, strip) pairs, workgroup g's range [units g / grid, units (g + 1) / grid): with more
    units than workgroups some ranges hold two units - a step from plane to plane - and one of them ends an item"""
    for cid, grid in G.ROW_OVER_GRID.items():
        c = G.BY_ID[cid]
        D, H, W = c.dims
        assert c.kernel.startswith('conv_row_kernel<4,') and W == 64 and H % 4 == 0 and H <= 64       # one strip per plane (pick_strips)
        lds = (2 if c.cin2 else 1) * 12 * (W + 2) * 32 + 4 * 16 * 2 * 8
        assert grid == 256 * min(160 * 1024 // lds, 2)
        units = c.n * D
        assert units > grid
        ranges = [(units * g // grid, units * (g + 1) // grid) for g in range(grid)]
        assert sum(b - a >= 2 for a, b in ranges) >= 1
        assert sum(b - a >= 2 and a // D != (b - 1) // D for a, b in ranges) >= 1


def test_committed_tconv_cases_meet_the_launch_rule_they_name():
    for c in G.DENSE_CASES:
        if c.kind != 'tconv':
            continue
        lds_w, row_store = G.TCONV_FLAGS[c.id]
        cp, nblk, taps = (c.cin + 15) // 16 * 16, (c.cout + 15) // 16, int(np.prod(c.stride))
        nbt = 2 if nblk % 2 == 0 else 1
        tg = min(taps, 4)
        assert c.kernel == f'tconv_mfma_kernel<{nbt},{tg}>'
        assert lds_w == ((cp + 31) // 32 >= 4 and 'FNN_TCONV_NO_LDSW' not in c.knobs)
        assert row_store == (c.stride[2] == 2 and nbt == 2 and tg % 2 == 0 and 'FNN_TCONV_NO_ROWSTORE' not in c.knobs)
    flags = {(c.kernel, G.TCONV_FLAGS[c.id]) for c in G.DENSE_CASES if c.kind == 'tconv'}
    # every combination the rule can reach: whole-row stores need two cout blocks (NBT = 2)
    for kernel in ('tconv_mfma_kernel<1,2>', 'tconv_mfma_kernel<1,4>'):
        assert {(kernel, (False, False)), (kernel, (True, False))} <= flags
    for kernel in ('tconv_mfma_kernel<2,2>', 'tconv_mfma_kernel<2,4>'):
        assert {(kernel, (lw, rw)) for lw in (False, True) for rw in (False, True)} <= flags
    assert {m for i in G.STORE_CASES if G.BY_ID[i].kind == 'tconv' for m in [G.TCONV_FLAGS[i][1]]} == {False, True}


@pytest.mark.parametrize('sc', G.STAGE_CASES, ids=lambda s: s.id)
def test_staging_sweeps_are_unambiguous_and_hold_the_edges(sc):
    x, gamma, beta, w = G.stage_data(sc)
    assert R.stage_params(x, (gamma, beta), margin=4.0)[3] == 0
    x = x.astype(np.float64)
    sc_h, sh_h, _, _ = R.stage_params(x, (gamma, beta))
    ex = (slice(None), slice(None), None, None, None)
    exact = x * sc_h[ex] + sh_h[ex]
    o = R.fma16(x, sc_h[ex], sh_h[ex])
    ties = np.abs(exact - o) == R.ulp16(o) / 2
    assert ties.sum() >= 20                                                               # fp16 ties of the fused multiply-add
    assert ((np.abs(o) < 2.0 ** -14) & (exact != 0)).sum() >= 1                             # cancellation into the subnormal range
    prod = o * B.h16(0.01)
    assert ((o < 0) & (np.abs(prod) < 2.0 ** -14)).sum() >= 20                              # slope products in the subnormal range
    assert (B.h16(B.h16(x * sc_h[ex]) + sh_h[ex]) != o).sum() >= 20                        # where two roundings differ from one
    want = G.stage_expected(sc, R.act16(o, 0.01))
    assert want.shape[1] == sc.cout and np.isfinite(want).all()
    if sc.kernel.startswith(G.FP32_STAGING):
        for slope in G.STAGE_SLOPES:
            v32, lo, hi, n_open = R.stage32(x, (gamma, beta), slope)
            v16 = R.stage16(x, (gamma, beta), slope)[0]
            assert n_open <= 1e-2 * x.size and (lo <= v32).all() and (v32 <= hi).all()
            assert ((v16 < lo) | (v16 > hi)).mean() > 0.05        # the fp16 form is another value on this data


# ---- sensitivity: mutants of the reference ------------------------------------------------------------------------------
def _differs(y, z):
    return not np.array_equal(G._bits(y), G._bits(z))


def _conv(case, a, d):
    return G.case_reference(case, d, a)[1]


def test_mutant_one_tap_dropped_at_a_ragged_tile_edge():
    case = G.BY_ID['lds-pad-8-24']
    d = G.case_data(case, 'ident')
    a = G.case_staged(d)[0]
    t, y16 = G.case_reference(case, d, a)
    n, co, od, oh, ow = 1, 17, 6, 8, 10                            # the last voxel: tiles of 4 x 8 x 8 end ragged at 7 x 9 x 11
    ci = int(np.flatnonzero(a[n, :, od, oh, ow - 1])[0])
    t2 = t.copy()
    t2[n, co, od, oh, ow] -= float(d['w'][co, ci, 1, 1, 0]) * a[n, ci, od, oh, ow - 1]
    assert _differs(y16, B.h16(t2))


def test_mutant_two_input_channels_swapped_inside_a_chunk():
    for cid in ('zr-2-8-zrp', 'tconv-1-4'):
        case = G.BY_ID[cid]
        d = G.case_data(case, 'ident')
        a = G.case_staged(d)[0]
        m = a.copy()
        m[:, [17 if case.cin > 17 else 1, 18 if case.cin > 18 else 2]] = m[:, [18 if case.cin > 18 else 2, 17 if case.cin > 17 else 1]]
        assert _differs(_conv(case, a, d), _conv(case, m, d))


def test_mutant_second_sources_norm_applied_to_the_first():
    case = G.BY_ID['zr-2-8-two-src']
    d = G.case_data(case, 'two')
    a = G.case_staged(d)[0]
    s2, h2, _, _ = R.stage_params(d['x2'], d['norm2'])
    ex = (slice(None), slice(None), None, None, None)
    wrong = R.act16(R.fma16(d['x'].astype(np.float64), s2[:, :case.cin][ex], h2[:, :case.cin][ex]), d['slope2'])
    m = np.concatenate((wrong, a[:, case.cin:]), 1)
    assert _differs(_conv(case, a, d), _conv(case, m, d))


def test_mutant_shift_applied_to_the_zero_padding():
    case = G.BY_ID['lds-pad-8-24']
    d = G.case_data(case, 'norm')
    a = G.case_staged(d)[0]
    _, sh_h, _, _ = R.stage_params(d['x'], d['norm'])
    fill = R.act16(sh_h, d['slope'])                               # what a zero voxel becomes when the shift reaches it
    padded = np.pad(a, ((0, 0), (0, 0), (1, 1), (1, 1), (1, 1)))
    border = np.pad(np.zeros(a.shape[2:]), 1, constant_values=1.0)
    padded = padded + border[None, None] * fill[:, :, None, None, None]
    m = F.conv3d(torch.from_numpy(padded), torch.from_numpy(d['w'].astype(np.float64)), torch.from_numpy(d['bias'].astype(np.float64))).numpy()
    assert _differs(_conv(case, a, d), B.h16(m))
    assert not _differs(_conv(case, a, d), B.h16(F.conv3d(torch.from_numpy(np.pad(a, ((0, 0), (0, 0), (1, 1), (1, 1), (1, 1)))), torch.from_numpy(d['w'].astype(np.float64)),
                                                          torch.from_numpy(d['bias'].astype(np.float64))).numpy()))


def test_mutants_of_the_staging_arithmetic():
    sc = G.STAGE_CASES[0]
    x, gamma, beta, _ = G.stage_data(sc)
    x = x.astype(np.float64)
    v = R.stage16(x, (gamma, beta), 0.01)[0]
    sc_h, sh_h, _, _ = R.stage_params(x, (gamma, beta))
    ex = (slice(None), slice(None), None, None, None)
    o = R.fma16(x, sc_h[ex], sh_h[ex])
    two = R.act16(B.h16(B.h16(x * sc_h[ex]) + sh_h[ex]), 0.01)                            # mul + add with two roundings
    assert _differs(v, two)
    f32 = np.maximum(o, B.h16(o * float(np.float32(0.01))))                               # the slope kept in fp32
    assert _differs(v, f32)
    with np.errstate(under='ignore'):
        fp32_form = B.h16((x * sc_h[ex] + sh_h[ex]).astype(np.float32))                   # the fp32 fma, then f16: rounds twice
    sc32, sh32, _, _ = B.scale_shift(x, gamma, beta)
    assert _differs(o, fp32_form) and _differs(o, B.h16(x * sc32[ex] + sh32[ex]))         # ... and with fp32 scale and shift


def test_mutant_eps_left_out():
    case = G.CONST_CASES[1]
    d = G.case_data(case, 'const')
    a = G.case_staged(d)[0]
    with np.errstate(divide='ignore', invalid='ignore'):
        s0, h0, _, _ = R.stage_params(d['x'], d['norm'], eps=0.0)
    s1, h1, _, _ = R.stage_params(d['x'], d['norm'])
    assert not np.array_equal(s0[:, 1], s1[:, 1])                  # the channel with one voxel different: var = 1.7e-4 against eps = 1e-5
    ex = (slice(None), slice(None), None, None, None)
    m = a.copy()
    m[:, 1] = R.act16(R.fma16(d['x'].astype(np.float64)[:, 1:2], s0[:, 1:2][ex], h0[:, 1:2][ex]), d['slope'])[:, 0]
    assert _differs(_conv(case, a, d), _conv(case, m, d))


def test_mutant_truncation_at_the_store():
    for mode in G.STORE_MODES:
        case = G.BY_ID['lds-pad-8-24']
        d = G.case_data(case, mode)
        t, y16 = G.case_reference(case, d)
        h = t.astype(np.float16)
        over = np.abs(h.astype(np.float64)) > np.abs(t)
        trunc = np.where(over, np.nextafter(h, np.float16(0)), h).astype(np.float64)
        assert _differs(y16, trunc)
