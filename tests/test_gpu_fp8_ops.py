"""Per-op parity of the e4m3 conv path on a real MI355X: conv3d_zr8_kernel<NB, TD> through fnn_op_conv3d with
FNN_OP_F8=1, against tests/fp8_ref.py - the path's defined arithmetic in float64 with torch's
float8_e4m3fn for every quantisation.  The network-level budgets (test_gpu_configs.py) cannot see a wrong per-cout
scale or bias - the InstanceNorm after every e4m3 conv cancels both - nor a local error that fits in 15 % RMSE.

The e4m3 choice takes a 3x3x3 stride-1 layer only at >= 480 workgroups (zr_choose); cases marked `knob` lower that
bound with FNN_ZR_MIN_WGS so that small layers (whose float64 reference stays cheap) reach the kernel, cases marked
`natural` are large enough without it."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import fp8_ref

pytestmark = pytest.mark.gpu


def _h(a):
    return torch.as_tensor(a).half().float()


def _pad16(c):
    return (c + 15) // 16 * 16


def _zr8_kernel(n, dims, cout, min_wgs=480):
    """the kernel zr_choose gives a 3x3x3 stride-1 layer with e4m3 operands (None: it refuses the layer)"""
    nblk = _pad16(cout) // 16
    nb = 2 if nblk % 2 == 0 else 1
    th, tw = -(-dims[1] // 8), -(-dims[2] // 8)
    td = 8
    while td >= 4 and (dims[0] < td or n * -(-dims[0] // td) * th * tw * (nblk // nb) < min_wgs):
        td -= 4
    return None if td < 4 else f'conv3d_zr8_kernel<{nb},{td}>'


@pytest.fixture
def f8(monkeypatch):
    monkeypatch.setenv('FNN_OP_F8', '1')
    monkeypatch.delenv('FNN_ZR_MIN_WGS', raising=False)
    return monkeypatch


def _run(f8, kernel, x, w, b, min_wgs=None, **kw):
    """one fnn_op_conv3d call with e4m3 operands; asserts the kernel that ran"""
    from fast_nnunet_amd import capi
    if min_wgs is None:
        f8.delenv('FNN_ZR_MIN_WGS', raising=False)
    else:
        f8.setenv('FNN_ZR_MIN_WGS', str(min_wgs))
    out = capi.op_conv3d(np.asarray(x, np.float32), np.asarray(w, np.float32), None if b is None else np.asarray(b, np.float32),
                         (3, 3, 3), (1, 1, 1), **kw)
    ran = capi.op_last_kernels()
    print(kernel, '->', ran)
    assert ran == [kernel], ran
    return out


def _check_stats(y, stats, what):
    y64 = y.astype(np.float64)
    assert np.allclose(stats[..., 0], y64.sum((2, 3, 4)), rtol=1e-6, atol=1e-3), what
    assert np.allclose(stats[..., 1], (y64 ** 2).sum((2, 3, 4)), rtol=1e-6, atol=1e-3), what


def _check_bracketed(y, ref, tol, uncertain, what):
    assert uncertain < 1e-3, f'{what}: {uncertain:.2e} of the activations sit on an e4m3 rounding boundary'
    assert np.isfinite(y).all(), what
    err = np.abs(y.astype(np.float64) - ref)
    bad = err > tol
    assert not bad.any(), (f'{what}: {int(bad.sum())} of {bad.size} outputs off, worst err {err.max():.4g} '
                           f'(tol there {tol.flat[int(np.argmax(err - tol))]:.3g}, ref max {np.abs(ref).max():.4g})')


# ---- the staging quantiser, read out exactly (knob: 8 workgroups)
@pytest.mark.parametrize('c', [16, 32])
def test_fp8_quantiser_reads_out_every_finite_fp16_value(f8, c):
    """Identity centre-tap weights (wq = 448 per cout, oscale = f32(1 / 448) / 8): acc = 448 q for the staged activation
    q, and q / 8 is an fp16 number, so 8 y = e4m3(clamp(8 x, +-448)) bit for bit for every finite fp16 x: ties to even,
    e4m3 subnormals (2^-9 .. 2^-6 after the x 8), saturation above 56, values that flush to zero.  The accumulator starts at
    +0, so a product of -0 reads out as +0: the reference's zeros are compared as +0."""
    bits = np.arange(1 << 16, dtype=np.uint32).astype(np.uint16)
    vals = bits.view(np.float16)
    vals = vals[np.isfinite(vals)].astype(np.float32)                      # 63488 values
    assert vals.size == 63488
    dims = (8, 256 // c, 31)                                                # c * 8 * (256 / c) * 31 = 63488
    x = vals.reshape(1, c, *dims)
    w = np.zeros((c, c, 3, 3, 3), np.float32)
    w[np.arange(c), np.arange(c), 1, 1, 1] = 1.0
    y = _run(f8, f'conv3d_zr8_kernel<{c // 16},8>', x, w, None, min_wgs=1)
    want = fp8_ref.e4m3(8.0 * x) / 8.0 + 0.0                                # (-0 -> +0)
    got_bits, want_bits = y.astype(np.float16).view(np.uint16), want.astype(np.float16).view(np.uint16)
    bad = got_bits != want_bits
    assert not bad.any(), (f'{int(bad.sum())} of {bad.size} values differ, e.g. x = {x[bad][:6]} -> 8y = '
                           f'{8 * y[bad][:6]}, e4m3 {8 * want[bad][:6]}')
    # what the readout covered: saturation, subnormals and ties (x = midpoints between e4m3 values / 8)
    q = 8.0 * want
    assert (np.abs(q) == 448).sum() > 1000 and ((np.abs(q) > 0) & (np.abs(q) < 2 ** -6)).sum() >= 14
    e = np.unique(np.abs(torch.arange(0, 127, dtype=torch.uint8).view(torch.float8_e4m3fn).double().numpy()))
    ties = np.isin(np.abs(8.0 * x), (e[1:] + e[:-1]) / 2)
    assert ties.sum() == 2 * 126                                           # every midpoint, both signs


# ---- operand map with exact numbers
OPMAP_CASES = [
    # n, cin, cin2, cout, dims, chunk-major, min_wgs (None: natural)
    (2, 16, 0, 16, (19, 13, 11), False, 1),        # <1,8> knob: ragged on every axis, n > 1
    (3, 32, 0, 32, (17, 10, 9), True, 1),          # <2,8> knob, chunk-major
    (2, 16, 16, 16, (6, 12, 20), False, 1),        # <1,4> knob: two sources
    (2, 8, 0, 24, (5, 9, 12), False, 1),           # <2,4> knob: padded channels on both sides (8 -> 16, 24 -> 32)
    (1, 8, 24, 24, (12, 10, 17), True, 1),         # <2,8> knob: two padded sources (3 chunks), chunk-major
    (3, 16, 0, 16, (36, 48, 50), False, None),     # <1,8> natural
    (30, 16, 0, 16, (4, 32, 32), True, None),      # <1,4> natural
    (4, 32, 0, 32, (40, 41, 39), False, None),     # <2,8> natural, ragged
    (12, 16, 16, 32, (7, 33, 31), True, None),     # <2,4> natural: two sources, chunk-major
]


@pytest.mark.parametrize('n,cin,cin2,cout,dims,cm,min_wgs', OPMAP_CASES, ids=lambda v: str(v).replace(' ', ''))
def test_fp8_operand_map_with_exact_numbers(f8, n, cin, cin2, cout, dims, cm, min_wgs):
    """Activations k / 8 (|k| <= 16: e4m3-exact after the x 8), one-hot and two-hot taps of weight 1 or 2 (max |w| 1 or 2 per
    cout: two different scales), bias an odd multiple of 1 / 16: every product and sum is exact, 1 / 16 <= |y| < 128, and the
    f32 rounding of the output scale stays far below half an fp16 ulp of y, so y must EQUAL F.conv3d - any permuted tap, depth
    shift, fragment lane, channel half, source, cout scale or padding value shows.  (An output that cancels to 0 would keep
    that rounding's residue: the odd sixteenth keeps every output away from 0.)"""
    if cm:
        f8.setenv('FNN_OP_CHUNK_MAJOR', '1')
    ctot = cin + cin2
    vox = np.arange(dims[0] * dims[1] * dims[2]).reshape(dims)
    x = np.stack([np.stack([((vox * 7 + ch * 3 + i * 5) % 33 - 16) / 8.0 for ch in range(ctot)]) for i in range(n)]).astype(np.float32)
    w = np.zeros((cout, ctot, 3, 3, 3), np.float32)
    for co in range(cout):
        if co % 3 != 2:
            w[co, (co * 5 + 3) % ctot, co % 3, (co // 3) % 3, (co + 1) % 3] = 1.0 + co % 3
        else:
            w[co, (co * 5 + 3) % ctot, co % 3, (co // 3) % 3, (co + 1) % 3] = 1.0
            w[co, (co * 3 + 1) % ctot, (co + 2) % 3, (co + 1) % 3, co % 3] += 2.0
    b = ((np.arange(cout) * 5 % 17) - 8) / 8.0 + 1 / 16.0
    kw = dict(x2=x[:, cin:]) if cin2 else {}
    y, stats = _run(f8, _zr8_kernel(n, dims, cout, min_wgs or 480), x[:, :cin], w, b, min_wgs, want_stats=True, **kw)
    ref = F.conv3d(torch.from_numpy(x), torch.from_numpy(w), torch.from_numpy(b.astype(np.float32)), 1, 1).numpy()
    assert np.abs(ref).max() < 128 and np.abs(ref).min() >= 1 / 16
    diff = y != ref
    assert not diff.any(), f'{int(diff.sum())} outputs differ, first at {np.argwhere(diff)[0]}: {y[diff][:4]} vs {ref[diff][:4]}'
    _check_stats(y, stats, 'operand map')


# ---- InstanceNorm + LeakyReLU on load (knob: small layers, float64 reference)
@pytest.mark.parametrize('two', [False, True])
def test_fp8_norm_and_leaky_relu_on_load(f8, two):
    """Per-item statistics that differ across the batch, slope 0.01; two sources where only the second is normalised (the
    decoder's case).  A few inputs sit beyond 56 sigma (the +-448 clamp), and many land in e4m3 subnormals after the slope."""
    g = torch.Generator().manual_seed(31 + two)
    n, c1, c2, cout, dims = 3, 16, 24, 24, (9, 12, 10)
    xs = []
    for c in ((c1, c2) if two else (c1,)):
        t = torch.randn(n, c, *dims, generator=g) * torch.tensor([0.5, 2.0, 7.0]).view(n, 1, 1, 1, 1) + \
            torch.tensor([1.0, -3.0, 0.25]).view(n, 1, 1, 1, 1)
        t.view(n, c, -1)[:, :, 0] = torch.tensor([1e3, -2e3, 4e3]).view(n, 1)      # a voxel far past 56 sigma
        xs.append(_h(t).numpy())
    ctot = sum(a.shape[1] for a in xs)
    w = _h(torch.randn(cout, ctot, 3, 3, 3, generator=g) / (ctot * 27) ** 0.5).numpy()
    b = torch.randn(cout, generator=g).numpy()
    normed = xs[-1]
    gamma, beta = (torch.rand(normed.shape[1], generator=g) + 0.5).numpy(), (torch.randn(normed.shape[1], generator=g) * 0.1).numpy()
    gamma[::4] = 3.0                                                        # (the outlier itself widens sigma to ~1/33 of it)
    if two:
        kw = dict(x2=xs[1], gamma2=gamma, beta2=beta, slope2=0.01)
        a = fp8_ref.act_bracket(xs[0])
        bq = fp8_ref.act_bracket(xs[1], (gamma, beta), 0.01)
        q = [np.concatenate((u, v), 1) for u, v in zip(a, bq)]
        chunks = 1 + _pad16(c2) // 16
    else:
        kw = dict(gamma=gamma, beta=beta, slope=0.01)
        q = bq = fp8_ref.act_bracket(xs[0], (gamma, beta), 0.01)
        chunks = 1
    qn = bq[0]
    assert (np.abs(qn) == 448).sum() >= n and ((qn != 0) & (np.abs(qn) < 2 ** -6)).sum() > 100
    y, stats = _run(f8, _zr8_kernel(n, dims, cout, 1), xs[0], w, b, 1, want_stats=True, **kw)
    ref, tol, unc = fp8_ref.conv_e4m3(*q, w, b, chunks=chunks)
    _check_bracketed(y, ref, tol, unc, f'norm on load, two sources {two}')
    _check_stats(y, stats, 'norm on load')


# ---- seeded random layers through the e4m3 rule (knob: FNN_ZR_MIN_WGS from the seed)
def _random_f8_layer(seed):
    rs = np.random.RandomState(3000 + seed)
    cin = int(rs.choice([8, 16, 21, 32, 48, 64]))
    two = cin % 16 == 0 and rs.rand() < 0.35
    cin2 = int(rs.choice([8, 16, 32])) if two else 0
    cout = int(rs.choice([10, 16, 24, 32, 48, 64]))
    n = int(rs.choice([1, 2, 3, 5]))
    dims = [int(rs.randint(4, 30)), int(rs.randint(3, 30)), int(rs.randint(3, 30))]
    while n * dims[0] * dims[1] * dims[2] * 27 * (cin + cin2) * cout > 6e8:
        i = int(np.argmax(dims))
        if dims[i] > 6:
            dims[i] = dims[i] * 3 // 4
        elif n > 1:
            n -= 1
        else:
            cout = max(16, cout // 2)
    min_wgs = int(rs.choice([1, 1, 4, 16, 64, 256]))
    while _zr8_kernel(n, dims, cout, min_wgs) is None:                    # (tile depth 4 where depth 8 has too few)
        min_wgs //= 4
    return n, cin, cin2, cout, tuple(dims), bool(rs.rand() < 0.5), bool(rs.rand() < 0.3), min_wgs


@pytest.mark.parametrize('seed', range(32))
def test_fp8_random_layers_against_the_e4m3_reference(f8, seed):
    """A 3x3x3 stride-1 layer drawn from a seed (odd planes, ragged tiles, channel padding, one or two sources, norm on load
    of the last source, chunk-major tensors) on the kernel the e4m3 rule gives it: the bracketed float64 reference and the
    epilogue statistics."""
    n, cin, cin2, cout, dims, norm, cm, min_wgs = _random_f8_layer(seed)
    kernel = _zr8_kernel(n, dims, cout, min_wgs)
    what = f'seed {seed}: n {n}, {cin}{"+" + str(cin2) if cin2 else ""} -> {cout}, {dims}, norm {norm}, cm {cm}, min_wgs {min_wgs}'
    assert kernel, what
    if cm:
        f8.setenv('FNN_OP_CHUNK_MAJOR', '1')
    g = torch.Generator().manual_seed(seed)
    x = _h(torch.randn(n, cin, *dims, generator=g) * 2 + 0.5).numpy()
    x2 = _h(torch.randn(n, cin2, *dims, generator=g) - 0.25).numpy() if cin2 else None
    ctot = cin + cin2
    w = _h(torch.randn(cout, ctot, 3, 3, 3, generator=g) / (ctot * 27) ** 0.5).numpy()
    b = torch.randn(cout, generator=g).numpy()
    last = x2 if cin2 else x
    nrm = None
    kw = {}
    if norm:
        nrm = ((torch.rand(last.shape[1], generator=g) + 0.5).numpy(), (torch.randn(last.shape[1], generator=g) * 0.1).numpy())
        kw = dict(gamma2=nrm[0], beta2=nrm[1], slope2=0.01) if cin2 else dict(gamma=nrm[0], beta=nrm[1], slope=0.01)
    if cin2:
        kw['x2'] = x2
    y, stats = _run(f8, kernel, x, w, b, min_wgs, want_stats=True, **kw)
    qa = fp8_ref.act_bracket(x, nrm if not cin2 else None, 0.01)
    if cin2:
        qb = fp8_ref.act_bracket(x2, nrm, 0.01)
        qa = [np.concatenate((u, v), 1) for u, v in zip(qa, qb)]
    ref, tol, unc = fp8_ref.conv_e4m3(*qa, w, b, chunks=(_pad16(cin) + _pad16(cin2)) // 16)
    _check_bracketed(y, ref, tol, unc, what)
    _check_stats(y, stats, what)


# ---- the weight scales' edges (knob)
def test_fp8_weight_scale_edges(f8):
    """Per-cout scales at their edges: an all-zero cout (output = bias), a cout dominated by one weight (the rest flush to
    e4m3 subnormals or zero), a cout whose max |w| = 1e-36 makes f32(max / 448) subnormal and 1 / ws infinite (it must give
    the bias, as the fp16 path does - not NaN), and padded couts (24 -> 32) that leave the real ones untouched: the same
    layer with 32 real couts gives the first 24 bit for bit."""
    g = torch.Generator().manual_seed(8)
    n, cin, dims = 2, 32, (10, 11, 9)
    x = _h(torch.randn(n, cin, *dims, generator=g)).numpy()
    w = _h(torch.randn(32, cin, 3, 3, 3, generator=g) / (cin * 27) ** 0.5).numpy()
    w[0] = 0
    w[1] *= 3e-4
    w[1, 5, 1, 1, 1] = 4.0
    w[2] = np.float32(1e-36) * np.sign(w[2]) * (np.abs(w[2]) > 0.05)
    w[3] *= 1e-30                                                          # tiny, but 1 / ws is finite
    w[24:] *= 64                                                           # scales far from the real couts'
    b = torch.randn(32, generator=g).numpy()
    wq, osc = fp8_ref.quantise_weights(w[:24])
    assert (wq[1] != 0).sum() < 0.5 * wq[1].size and ((wq[1] != 0) & (np.abs(wq[1]) < 2 ** -6)).any()
    y, stats = _run(f8, 'conv3d_zr8_kernel<2,8>', x, w[:24], b[:24], 1, want_stats=True)
    assert np.isfinite(y).all()
    for co in (0, 2):
        assert (y[:, co] == np.float16(b[co]).astype(np.float32)).all(), co
    ref, tol, unc = fp8_ref.conv_e4m3(*fp8_ref.act_bracket(x), w[:24], b[:24], chunks=2)
    _check_bracketed(y, ref, tol, unc, 'weight scale edges')
    _check_stats(y, stats, 'weight scale edges')
    y32 = _run(f8, 'conv3d_zr8_kernel<2,8>', x, w, b, 1)
    assert np.array_equal(y32[:, :24].view(np.uint32), y.view(np.uint32))


# ---- the fallback rule: layers the e4m3 choice refuses run their fp16 kernel
FALLBACK_CASES = [
    # n, cin, cout, dims, k, stride, min_wgs
    (2, 16, 16, (3, 20, 20), (3, 3, 3), (1, 1, 1), 1),          # Do < 4
    (2, 16, 32, (8, 20, 20), (1, 3, 3), (1, 1, 1), 1),          # (1, 3, 3) kernel
    (2, 32, 32, (16, 24, 24), (3, 3, 3), (1, 2, 2), 1),         # in-plane stride 2
    (1, 16, 16, (16, 16, 16), (3, 3, 3), (1, 1, 1), None),      # too few workgroups without the knob
    (2, 16, 16, (8, 16, 16), (3, 3, 3), (2, 2, 2), 1),          # stride 2
]


@pytest.mark.parametrize('n,cin,cout,dims,k,stride,min_wgs', FALLBACK_CASES, ids=lambda v: str(v).replace(' ', ''))
def test_fp8_fallback_runs_the_fp16_kernel(f8, n, cin, cout, dims, k, stride, min_wgs):
    from fast_nnunet_amd import capi
    if min_wgs is not None:
        f8.setenv('FNN_ZR_MIN_WGS', str(min_wgs))
    g = torch.Generator().manual_seed(n + cin + dims[0])
    x = _h(torch.randn(n, cin, *dims, generator=g)).numpy()
    w = _h(torch.randn(cout, cin, *k, generator=g) / (cin * 27) ** 0.5).numpy()
    b = torch.randn(cout, generator=g).numpy()
    y8, s8 = capi.op_conv3d(x, w, b, k, stride, want_stats=True)
    k8 = capi.op_last_kernels()
    f8.delenv('FNN_OP_F8')
    y16, s16 = capi.op_conv3d(x, w, b, k, stride, want_stats=True)
    k16 = capi.op_last_kernels()
    print(k8, k16)
    assert k8 == k16 and not any('zr8' in s for s in k8), (k8, k16)
    assert np.array_equal(y8.view(np.uint32), y16.view(np.uint32))
    assert np.allclose(s8, s16, rtol=1e-9, atol=1e-6)
