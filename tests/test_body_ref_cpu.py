"""tests/body_ref.py against the oracle and against hand-made values (no GPU): the float64 values the op tests compare the
device with are the oracle's operations, not a restatement of the kernels, and the bound helpers price a rounding right."""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import body_ref as R  # noqa: E402
from oracle.unet import ResBlock  # noqa: E402


def _close(got, want):
    """float64 roundoff: 1e-12 of the tensor's largest magnitude"""
    want = want.detach().numpy()
    assert got.shape == want.shape
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max(), np.abs(got - want).max()


def _conv_raw_and_norm(cna, x):
    """a ConvNormAct's raw conv output (double) and its InstanceNorm as body_ref's exact (scale, shift)"""
    raw = cna.conv(x).detach().numpy()
    return raw, R.scale_shift(raw, cna.norm.weight.detach().numpy(), cna.norm.bias.detach().numpy(), eps=cna.norm.eps, exact=True)


def _block(cin, cout, stride, seed):
    torch.manual_seed(seed)
    blk = ResBlock(cin, cout, (3, 3, 3), stride, True, 1e-5, 0.01).double().eval()
    with torch.no_grad():
        for name, p in blk.named_parameters():
            if 'norm' in name:
                p.copy_(torch.rand_like(p) + 0.5 if name.endswith('weight') else torch.randn_like(p) * 0.3)
    x = torch.randn(2, cin, 6, 8, 10, dtype=torch.float64) * 1.5 + 0.7
    return blk, x


def test_pool_combine_compose_to_the_oracles_strided_projecting_block():
    blk, x = _block(5, 7, (2, 2, 2), 1)
    h = blk.conv1(x)
    a, ss_a = _conv_raw_and_norm(blk.conv2, h)
    pooled, _ = R.pool(*R.transform(x.numpy()), (2, 2, 2))                   # skip: AvgPool3d, then 1x1x1 conv + norm
    b, ss_b = _conv_raw_and_norm(blk.skip[1], torch.from_numpy(pooled))
    t, _ = R.combine(a, b, 0.01, ss_a=ss_a, ss_b=ss_b)
    _close(t, F.leaky_relu(blk.conv2(h) + blk.skip(x), float(np.float32(0.01))))


def test_pool_combine_compose_to_the_oracles_identity_strided_block():
    """cin == cout, stride (1, 2, 2): the skip is the pooled block input itself, no norm behind it - where a wrong pooling
    divisor is not cancelled by an InstanceNorm"""
    blk, x = _block(6, 6, (1, 2, 2), 2)
    h = blk.conv1(x)
    a, ss_a = _conv_raw_and_norm(blk.conv2, h)
    b, _ = R.pool(*R.transform(x.numpy()), (1, 2, 2))
    t, _ = R.combine(a, b, 0.01, ss_a=ss_a)
    _close(t, F.leaky_relu(blk.conv2(h) + blk.skip(x), float(np.float32(0.01))))
    # an operand that is a raw conv output with norm AND activation (conv1's output as a later block's skip)
    raw, ss = _conv_raw_and_norm(blk.conv1, x)
    y, _ = R.transform(raw, ss, 0.01)
    _close(y, F.leaky_relu(blk.conv1.norm(blk.conv1.conv(x)), float(np.float32(0.01))))


def test_pooled_of_output_is_avgpool_of_the_block_output():
    y = np.random.default_rng(3).standard_normal((2, 3, 4, 6, 6))
    t, _ = R.pooled_of_output(y, (2, 2, 2))
    _close(t, F.avg_pool3d(torch.from_numpy(y), (2, 2, 2)))
    t, _ = R.pooled_of_output(y, (3, 1, 1))                                   # truncated like AvgPool3d: 4 // 3 = 1
    _close(t, F.avg_pool3d(torch.from_numpy(y), (3, 1, 1)))


def test_head_is_the_oracles_seg_layer():
    torch.manual_seed(4)
    seg = torch.nn.Conv3d(12, 5, 1, 1, 0, bias=True).double()
    x = torch.randn(1, 12, 3, 4, 5, dtype=torch.float64)
    t, _ = R.head(x[0].reshape(12, -1).numpy(), seg.weight.detach().numpy().reshape(5, 12), None)
    t = t + seg.bias.detach().numpy()[:, None]            # (head() rounds its bias to fp32: added here in double)
    _close(t.reshape(1, 5, 3, 4, 5), seg(x))
    # ... and with the bias through head(): fp32-representable values pass unchanged
    b = np.array([0.5, -1.25, 3.0, 0.0, 2.0 ** -20])
    t2, _ = R.head(x[0].reshape(12, -1).numpy(), seg.weight.detach().numpy().reshape(5, 12), b)
    _close(t2.reshape(1, 5, 3, 4, 5), F.conv3d(x, seg.weight, torch.from_numpy(b)))


def test_head_operand_on_hand_made_values():
    x = np.array([[[1.0, -2.0, 0.0, 1.0 + 2.0 ** -10]]])                       # [1, 1, 4]
    o, spread = R.head_operand(x, None, 0.01)
    s16 = float(np.float16(0.01))
    assert o.tolist() == [[[1.0, float(np.float16(-2.0 * s16)), 0.0, 1.0 + 2.0 ** -10]]] and not spread.any()
    # scale 3, shift 0.5 known exactly: (1 + 2^-10) * 3 + 0.5 = 3.5 + 3 * 2^-10 rounds to fp16 once (spacing 2^-9 there: a tie
    # between 3.5 + 2^-9 and 3.5 + 2^-8, to the even one)
    ss = (np.array([[3.0]]), np.array([[0.5]]), np.zeros((1, 1)), np.zeros((1, 1)))
    o, spread = R.head_operand(x, ss, 1.0)
    assert o.tolist() == [[[3.5, -5.5, 0.5, 3.5 + 2.0 ** -8]]] and not spread.any()
    # a scale on an fp16 rounding boundary (1 + 2^-11, known to +-2^-20): both roundings are covered by the spread
    ss = (np.array([[1.0 + 2.0 ** -11]]), np.zeros((1, 1)), np.full((1, 1), 2.0 ** -20), np.zeros((1, 1)))
    o, spread = R.head_operand(np.array([[[1024.0]]]), ss, 1.0)
    assert spread.item() == 1.0 and o.item() in (1024.0, 1025.0)
    t, e = R.head(np.array([[2.0]]), np.array([[0.5]]), None, np.array([[1.0]]))
    assert t.item() == 1.0 and e.item() == 33 * R.U32 * 1.0 + 0.5


def test_unflip_and_first_mask():
    t = np.arange(2 * 24, dtype=np.float64).reshape(2, 24)
    u = R.unflip(t, (2, 3, 4), (1, 0, 1)).reshape(2, 2, 3, 4)
    assert u[1, 0, 2, 0] == t.reshape(2, 2, 3, 4)[1, 1, 2, 3]
    m = R.first_mask((2, 3, 4), (1, 0, 2))
    assert m.sum() == 1 * 3 * 2 and m[1, 0, 2] and not m[0, 2, 3] and not m[1, 2, 1]
    assert R.first_mask((2, 3, 4), (0, 0, 0)).all() and not R.first_mask((2, 3, 4), (R.INT_MAX,) * 3).any()


def test_half_ulp16_on_hand_made_values():
    # 1.0: spacing 2^-10 above, half of it 2^-11; just below 1 the spacing halves
    assert R.half_ulp16(1.0) == 2.0 ** -11 and R.half_ulp16(0.999) == 2.0 ** -12
    assert R.half_ulp16(2047.0) == 0.5 and R.half_ulp16(2048.0) == 1.0
    # zero and subnormals: spacing 2^-24 throughout; the smallest normal 2^-14 has the same spacing
    assert R.half_ulp16(0.0) == 2.0 ** -25 and R.half_ulp16(2.0 ** -24) == 2.0 ** -25 and R.half_ulp16(2.0 ** -14) == 2.0 ** -25
    assert R.half_ulp16(2.0 ** -13) == 2.0 ** -24
    # a tie: 1 + 2^-11 lies half way between 1 and 1 + 2^-10; whichever way it goes the error is exactly the bound
    tie = 1.0 + 2.0 ** -11
    assert abs(float(np.float16(tie)) - tie) == R.half_ulp16(tie) and float(np.float16(tie)) == 1.0      # to even
    # every fp16 rounding of a spread of magnitudes stays inside the bound, and the bound is attained somewhere
    v = np.random.default_rng(0).standard_normal(200000) * np.logspace(-8, 4, 200000)
    err = np.abs(R.h16(v) - v.astype(np.float32).astype(np.float64))
    assert (err <= R.half_ulp16(v)).all() and (err > 0.99 * R.half_ulp16(v)).any()
    assert (R.store16(np.array([1.0]), np.array([0.25])) == 0.25 + 2.0 ** -11).all()


def test_transform_and_pool_bounds_on_hand_made_values():
    x = np.array([[[[[0.0, 2.0, -3.0, 0.5]]]]])                               # [1, 1, 1, 1, 4]
    y, e = R.transform(x)                                                     # identity: the values themselves, no error
    assert (y == x).all() and (e == 0).all()
    y, e = R.transform(x, None, 0.01)
    s = float(np.float32(0.01))
    assert y[0, 0, 0, 0, 2] == -3.0 * s and e[0, 0, 0, 0, 2] == R.U32 * 3.0 * s and e[0, 0, 0, 0, 0] == 0
    ss = (np.array([[2.0]]), np.array([[1.0]]), np.array([[0.0]]), np.array([[0.0]]))
    y, e = R.transform(x, ss)
    assert (y == 2 * x + 1).all() and (e == R.U32 * np.abs(2 * x + 1)).all()   # exact (sc, sh): the fma's own rounding only
    t, e = R.pool(np.abs(x), 0.0, (1, 1, 4))
    assert t.item() == 5.5 / 4 and e.item() == 5 * R.U32 * 5.5 / 4
    # a zero tensor: nothing to round but the store's subnormal half spacing
    t, b = R.combine(np.zeros((1, 1, 1, 1, 2)), np.zeros((1, 1, 1, 1, 2)), 0.01)
    assert (t == 0).all() and (b == 2.0 ** -25).all()


def test_scale_shift_error_terms():
    x = R.h16(np.random.default_rng(1).standard_normal((2, 3, 4, 4, 4)) * 0.5 + 4.0)
    gamma, beta = np.array([1.0, 0.5, 2.0], np.float32), np.array([0.0, 0.1, -1.0], np.float32)
    sc, sh, e_sc, e_sh = R.scale_shift(x, gamma, beta)
    xs, _, _, _ = R.scale_shift(x, gamma, beta, exact=True)
    assert np.abs(sc - xs).max() < 1e-5 * np.abs(sc).max()                    # (the fp32 count reciprocal and eps)
    assert (e_sc == 2 * R.U32 * np.abs(sc)).all()
    mean = x.reshape(2, 3, -1).mean(2)
    assert np.allclose(e_sh, R.U32 * (5 * np.abs(mean * sc) + np.abs(beta)[None]), rtol=1e-6)
    # the fp32 arithmetic of the kernel, restated in numpy float32, lies inside the stated errors
    inv = np.float32(1) / np.float32(64)
    m64 = x.reshape(2, 3, -1).sum(2) * float(inv)
    v64 = np.maximum((x.reshape(2, 3, -1) ** 2).sum(2) * float(inv) - m64 * m64, 0)
    rstd = (1.0 / np.sqrt(v64 + float(np.float32(1e-5)))).astype(np.float32)
    sc32 = gamma[None] * rstd
    sh32 = beta[None] - m64.astype(np.float32) * sc32
    assert (np.abs(sc32.astype(np.float64) - sc) <= e_sc).all() and (np.abs(sh32.astype(np.float64) - sh) <= e_sh).all()


def test_accumulate_and_weight_channel_and_patch_input():
    one = np.array([0x3C00, 0x0001], np.uint16)                               # 1.0 and the smallest fp16 subnormal
    w = R.weight_channel(np.array([0.0, 0.0], np.float16), one, False)
    assert w.dtype == np.float16 and w.view(np.uint16).tolist() == [0x3C00, 0x0001]       # the subnormal weight survives
    w = R.weight_channel(np.array([np.nan, 2.0], np.float32), one, True, first=np.array([True, False]))
    assert w.dtype == np.float32 and w[0] == 1.0 and w[1] == np.float32(2.0) + np.float32(2.0 ** -24)
    t, e_t = np.array([[3.0, -2.0]]), np.array([[0.0, 0.0]])
    s, e = R.accumulate(np.array([[np.nan, 1.0]]), t, e_t, np.array([0.5, 2.0]), True, first=np.array([True, False]))
    assert s.tolist() == [[1.5, -3.0]] and e.tolist() == [[2 * R.U32 * 1.5, R.U32 * (4.0 + 3.0)]]
    _, e16 = R.accumulate(np.array([[0.0, 1.0]]), t, e_t, np.array([0.5, 2.0]), False)
    assert e16[0, 1] == R.U32 * 7.0 + R.half_ulp16(3.0 + R.U32 * 7.0)
    vol = np.array([70000.0, 2.0 ** -25, 2.0 ** -24 * 1.5, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, -65520.0], np.float32).reshape(1, 1, 1, 6)
    bits = R.patch_input(vol, [[0, 0, 0]], (1, 1, 6), 16, (0, 0, 0))
    # overflow -> inf; a tie at half the smallest subnormal -> 0 (even); 1.5 subnormal units -> 2 units (even); the two ties
    # around 1 + 2^-10 go to even mantissas; -65520 is the tie that rounds to -inf
    assert bits[0, 0, 0, 0].tolist() == [0x7C00, 0x0000, 0x0002, 0x3C00, 0x3C02, 0xFC00] and not bits[0, 1:].any()
    assert R.patch_input(vol, [[0, 0, 2]], (1, 1, 3), 16, (0, 0, 1))[0, 0, 0, 0].tolist() == [0x3C02, 0x3C00, 0x0002]


def test_h16_rounds_a_float64_once():
    # 1 + 2^-11 + 2^-30 lies above the tie between 1 and 1 + 2^-10; float32 would first round it onto the tie, then to even
    v = 1.0 + 2.0 ** -11 + 2.0 ** -30
    assert float(np.float32(v)) == 1.0 + 2.0 ** -11 and R.h16(v) == 1.0 + 2.0 ** -10
