"""The paired k-step order of conv3d_zr_kernel (FNN_PACK_ZRP): the leftover in-plane tap 8 of two consecutive 16-channel
chunks shares one k-step, 27 k-steps per 32 input channels instead of 30.  The CPU test pins the operand map of the host
packer; the GPU tests compare the paired kernel with its padded order (FNN_NO_ZRP) bit for bit on small integers, where
fp32 accumulation is exact in either order, and against torch within the op tolerance."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

PACK_ZR, PACK_ZRP = 1, 3


@pytest.fixture(scope='module')
def kstep_tap():
    from fast_nnunet_amd import capi
    lib = capi.load_library()
    f = getattr(lib, '_Z16conv3d_kstep_tapiiiiiiPi')      # int conv3d_kstep_tap(packing, ks, half, taps, ch, chunks, int *tch)
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_int] * 6 + [ctypes.POINTER(ctypes.c_int)]

    def call(packing, ks, half, ch, chunks):
        tch = ctypes.c_int(-7)
        tap = f(packing, ks, half, 27, ch, chunks, ctypes.byref(tch))
        return tap, tch.value
    return call


@pytest.mark.parametrize('chunks', [1, 2, 3, 4, 5, 8])
def test_paired_kstep_map_covers_every_tap_once(kstep_tap, chunks):
    """Every (chunk, tap) of the layer sits in exactly one k-step half; the shared k-steps hold tap 8 of both chunks of a pair."""
    for packing in (PACK_ZR, PACK_ZRP):
        seen = {}
        pads = 0
        for ch in range(chunks):
            for ks in range(15):
                for half in range(2):
                    tap, tch = kstep_tap(packing, ks, half, ch, chunks)
                    if tap < 0:
                        pads += 1
                        continue
                    assert 0 <= tap < 27 and 0 <= tch < chunks
                    if ks < 12:                             # tap pairs 0 .. 3 of the chunk itself, depth offset ks % 3
                        assert (tap, tch) == ((ks % 3) * 9 + 2 * (ks // 3) + half, ch)
                    else:
                        assert tap == (ks % 3) * 9 + 8
                    key = (tch, tap)
                    assert key not in seen, (packing, key, seen.get(key), (ch, ks, half))
                    seen[key] = (ch, ks, half)
        assert len(seen) == 27 * chunks
        # 30 halves per chunk for 27 taps in both orders; in the paired one the zero halves are the first chunk's three
        # k-steps, which the kernel does not multiply: 27 k-steps per pair instead of 30
        assert pads == 3 * chunks
        if packing == PACK_ZRP:
            for c in range(0, chunks - 1, 2):                     # the shared k-steps: half 0 chunk c, half 1 chunk c + 1
                for dz in range(3):
                    assert kstep_tap(PACK_ZRP, 12 + dz, 0, c + 1, chunks) == (dz * 9 + 8, c)
                    assert kstep_tap(PACK_ZRP, 12 + dz, 1, c + 1, chunks) == (dz * 9 + 8, c + 1)
                    assert kstep_tap(PACK_ZRP, 12 + dz, 0, c, chunks)[0] == -1


def _h(a):
    return torch.as_tensor(a).half().float()


def _zr_kernel(names):
    return len(names) == 1 and names[0] in ('conv3d_zr_kernel<2,8>', 'conv3d_zr_kernel<1,8>', 'conv3d_zr_kernel<2,4>',
                                            'conv3d_zr_kernel<1,4>')


# (n, cin, cin2, cout, dims): 2 .. 5 chunks; a two-source layer whose pair (2, 3) straddles the sources (48 + 32); ragged
# tiles along d, h and w; one and two cout blocks per workgroup
CASES = [(18, 32, 0, 32, (20, 17, 23)),
         (27, 48, 0, 32, (19, 20, 13)),
         (12, 64, 0, 48, (21, 15, 18)),
         (18, 80, 0, 32, (20, 17, 23)),
         (18, 48, 32, 32, (18, 19, 22)),
         (9, 24, 40, 64, (13, 20, 17))]


@pytest.mark.gpu
@pytest.mark.parametrize('n,cin,cin2,cout,dims', CASES)
def test_conv3d_zr_paired_matches_padded_order(n, cin, cin2, cout, dims, monkeypatch):
    from fast_nnunet_amd import capi
    monkeypatch.delenv('FNN_NO_ZRP', raising=False)
    ctot = cin + cin2
    # small integers: every partial sum is exact in fp32, so the two k orders must give the same bits
    gi = torch.Generator().manual_seed(5 + ctot + dims[0])
    xi = torch.randint(-3, 4, (n, cin, *dims), generator=gi).float()
    wi = torch.randint(-2, 3, (cout, ctot, 3, 3, 3), generator=gi).float()
    kw = {}
    if cin2:
        x2i = torch.randint(-3, 4, (n, cin2, *dims), generator=gi).float()
        kw = dict(x2=x2i.numpy())
    y = capi.op_conv3d(xi.numpy(), wi.numpy(), None, (3, 3, 3), (1, 1, 1), **kw)
    names = capi.op_last_kernels()
    assert _zr_kernel(names), names
    monkeypatch.setenv('FNN_NO_ZRP', '1')
    y_pad = capi.op_conv3d(xi.numpy(), wi.numpy(), None, (3, 3, 3), (1, 1, 1), **kw)
    assert capi.op_last_kernels() == names
    monkeypatch.delenv('FNN_NO_ZRP')
    assert np.array_equal(y.view(np.uint16), y_pad.view(np.uint16))
    ref = F.conv3d(xi if not cin2 else torch.cat((xi, x2i), 1), wi, None, 1, 1)
    assert np.array_equal(y, _h(ref).numpy())

    # real data with the fused normalisation: the op tolerance, statistics rows against float64 sums
    g = torch.Generator().manual_seed(31 + ctot + cout)
    x = _h(torch.randn(n, cin, *dims, generator=g) * 2 + 0.5)
    gamma, beta = torch.rand(cin, generator=g) + 0.5, torch.randn(cin, generator=g) * 0.1
    w = _h(torch.randn(cout, ctot, 3, 3, 3, generator=g) / (ctot * 27) ** 0.5)
    b = torch.randn(cout, generator=g)
    kw = dict(gamma=gamma.numpy(), beta=beta.numpy(), slope=0.01, want_stats=True)
    x2 = None
    if cin2:
        x2 = _h(torch.randn(n, cin2, *dims, generator=g))
        kw.update(x2=x2.numpy())
    y, stats = capi.op_conv3d(x.numpy(), w.numpy(), b.numpy(), (3, 3, 3), (1, 1, 1), **kw)
    assert capi.op_last_kernels() == names
    xn = _h(F.leaky_relu(F.instance_norm(x, weight=gamma, bias=beta, eps=1e-5), 0.01))
    ref = F.conv3d(xn if x2 is None else torch.cat((xn, x2), 1), w, b, 1, 1)
    assert np.abs(y - ref.numpy()).max() <= 6e-3 * max(1.0, float(ref.abs().max()))
    y64 = y.astype(np.float64)
    assert np.allclose(stats[..., 0], y64.sum((2, 3, 4)), rtol=1e-6, atol=1e-3)
    assert np.allclose(stats[..., 1], (y64 ** 2).sum((2, 3, 4)), rtol=1e-6, atol=1e-3)
