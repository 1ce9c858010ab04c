"""float64 restatement of the f16 conv and transposed-conv path (csrc/conv3d*.hip, conv2d_zp.hip, conv3d_row.hip, tconv.hip)
that tests/test_gpu_conv_exact.py and tests/test_gpu_stem_fused_exact.py compare the device with BIT FOR BIT.  Plain numpy and torch CPU, no device code.

The route is data on which the kernels' arithmetic is exact, so that there is one right answer whatever the order of the
fp32 sums: fits_exact / stats_fit_exact say when that holds.  Roundings restated, and where they are made:

  staging (stage16)      fnn_device.h fnn_norm8 + conv_common.h fnn_norm_leaky8 + act_load.h norm_act_frag:
                           sc_h = f16(sc), sh_h = f16(sh)        stats_finalize_kernel's ssh rows (body.hip) hold the same roundings
                           o = f16(x * sc_h + sh_h)              ONE rounding: `x * sc_h + sh_h` on f16x8 contracts to v_pk_fma_f16
                           max(o, f16(o * f16(slope)))           v_pk_mul_f16, v_pk_max_f16
                         (sc, sh): stats_finalize_kernel, restated by body_ref.scale_shift (float64 sums, the wrapper's
                         f32(1 / voxels), the fp32 eps); they are known to within (e_sc, e_sh), so the fp16 rounding of one
                         that sits on a rounding boundary is ambiguous - stage16 counts those and brackets the value.
                         max(o, o * slope) is LeakyReLU only for 0 <= slope <= 1: beyond that range it picks the other branch.
  staging (stage32)      conv3d.hip conv3d_mfma_kernel and conv3d_lds_kernel, the two kernels that do NOT go through fnn_norm8:
                           o = f16(fma32(x, sc, sh)) on the fp32 rows, then the same max(o, f16(o * f16(slope))).
                         With fp32 (sc, sh) known only to within (e_sc, e_sh) the value is a bracket per element, not a number:
                         the device must lie inside it (it is one fp16 value for all but a few elements in a thousand).
  accumulation           v_mfma_f32_16x16x32_f16 chains in fp32 from +0 or from the bias: products of two fp16 numbers are
                         exact in fp32; every partial sum is exact when fits_exact holds.
  store                  conv_common.h tile_epilogue (and each family's own): f16(acc + bias), one rounding of the exact value
                         when fits_exact holds -> conv_exact / tconv_exact round the float64 result straight to fp16.
  stem (stem_exact)      conv3d_thin.hip / conv3d_row.hip: the patch window of the fp32 volume, mirrored, x and w rounded to fp16,
                         zero padding at the PATCH border, then accumulation and store as above.  A fused consumer recomputes
                         exactly these stored values (f16 of the stem's sum) before it normalises them: fused_stem_staged.
  fused transposed conv  conv3d_thin.hip / conv3d_row.hip: "up" = f16(tconv(stage16(low)) + bias), the bits tconv_mfma_kernel
                         stores, concatenated in front of the staged skip: fused_tconv_staged.
  statistics             tile_epilogue's v_dot2_f32_f16 chains, row16_sum, the workgroup sum in double, replica atomics or
                         slot rows, fnn_op_conv3d's sum over the rows: sums of the fp16-rounded outputs - integers in units of
                         the outputs' quantum, exact in every order when stats_fit_exact holds.
"""
import numpy as np
import torch
import torch.nn.functional as F

from body_ref import U32, h16, scale_shift

F16_TARGETS = ((0.5, 1.0), (0.25, -3.0), (1.5, 2.0), (0.125, 0.5))     # (S, H) pairs craft_norm is checked on (test_conv_ref_cpu.py)


def _ex(a, ndim):
    return np.asarray(a)[(slice(None), slice(None)) + (None,) * (ndim - 2)]


def ulp16(v):
    """spacing of fp16 at |v| (float64): every fp16 number is a multiple of it"""
    with np.errstate(over='ignore'):
        return np.spacing(np.abs(np.asarray(v, np.float64)).astype(np.float16)).astype(np.float64)


def quantum(*arrays):
    """the largest power of two that divides every non-zero value of the arrays (float64); 1.0 if all are zero"""
    q = None
    for a in arrays:
        a = np.asarray(a, np.float64).ravel()
        a = a[a != 0]
        if a.size == 0:
            continue
        m, e = np.frexp(a)                                  # a = m 2^e, 0.5 <= |m| < 1: m 2^53 is an integer
        mi = np.abs(m * 2.0 ** 53).astype(np.int64)
        low = np.log2((mi & -mi).astype(np.float64)).astype(np.int64)     # its lowest set bit
        k = int((e.astype(np.int64) - 53 + low).min())
        q = k if q is None else min(q, k)
    return 1.0 if q is None else float(np.ldexp(1.0, q))


def stage_params(x, norm, eps=1e-5, margin=1.0):
    """The fp16 (scale, shift) rows of the normalise-on-load of x [n, c, ...] -> (sc_h, sh_h, corners, ambiguous): sc_h, sh_h
    [n, c] float64 holding fp16 values, corners = the four (sc_h, sh_h) pairs at the ends of body_ref's intervals
    sc +- margin e_sc, sh +- margin e_sh, ambiguous = the number of (item, channel) pairs where a corner differs from the
    centre, i.e. whose fp16 rounding the last bits of the kernel's fp32 value decide."""
    sc, sh, e_sc, e_sh = scale_shift(x, norm[0], norm[1], eps=eps)
    sc_h, sh_h = h16(sc), h16(sh)
    corners = [(h16(sc + a * margin * e_sc), h16(sh + b * margin * e_sh)) for a in (-1, 1) for b in (-1, 1)]
    amb = np.zeros(sc.shape, bool)
    for s, h in corners:
        amb |= (s != sc_h) | (h != sh_h)
    return sc_h, sh_h, corners, int(amb.sum())


def span_ok(x, s, h):
    """the exponent-span condition of fma16, per element: product and addend are both multiples of
    q = min(ulp16(x) ulp16(s), ulp16(h)) (over the non-zero ones), and (|x s| + |h|) / q < 2^53 - one 53-bit window"""
    p = x * s + np.zeros_like(h)
    q = np.minimum(np.where(p != 0, ulp16(x) * ulp16(s), np.inf), np.where(h + np.zeros_like(p) != 0, ulp16(h), np.inf))
    q = np.where(np.isfinite(q), q, 1.0)
    return (np.abs(p) + np.abs(h)) / q < 2.0 ** 53


def fma16(x, s, h):
    """f16(x * s + h) with ONE rounding for fp16-valued float64 arrays.  x * s is exact in float64 (22 significant bits);
    the sum is exact in float64 under span_ok's condition (asserted: it holds for operands within about 30 binades of each
    other, as everything a network or a test here stages is), and is then rounded to fp16 once."""
    assert span_ok(x, s, h).all(), 'x * s + h is not exact in float64 for these magnitudes'
    return h16(x * s + h)


def act16(o, slope):
    """max(o, f16(o * f16(slope))): the product of two fp16 numbers is exact in float64, one rounding"""
    return np.maximum(o, h16(o * h16(slope)))


def stage16(x, norm=None, slope=1.0, eps=1e-5, margin=1.0):
    """The staged activation a conv / transposed conv multiplies, for the raw fp16-valued tensor x [n, c, ...] ->
    (value, lo, hi, ambiguous).  norm = None: x itself (the launchers pass slope 1 with the identity rows).  norm = (gamma,
    beta) [c]: max(o, f16(o * f16(slope))) with o = f16(x * f16(sc) + f16(sh)).  lo / hi: the extremes over the four corners
    of stage_params (equal to the value wherever nothing is ambiguous); ambiguous: stage_params' count."""
    x = np.asarray(x, np.float64)
    if norm is None:
        return x, x, x, 0
    sc_h, sh_h, corners, amb = stage_params(x, norm, eps, margin)
    def op(s, h):                                        # item by item: the temporaries of a batch of patches stay small
        return np.stack([act16(fma16(x[i:i + 1], _ex(s[i:i + 1], x.ndim), _ex(h[i:i + 1], x.ndim)), slope)[0] for i in range(x.shape[0])])
    v = op(sc_h, sh_h)
    if amb == 0:
        return v, v, v, 0
    cands = [op(s, h) for s, h in corners] + [v]
    return v, np.minimum.reduce(cands), np.maximum.reduce(cands), amb


def stage32(x, norm, slope=1.0, eps=1e-5):
    """The staged activation of the kernels that normalise with the fp32 rows (conv3d_mfma_kernel, conv3d_lds_kernel):
    max(o, f16(o * f16(slope))) with o = f16(fma32(x, sc, sh)) -> (value, lo, hi, open).  z = x sc + sh is increasing in sh and
    monotone in sc, so over sc +- e_sc, sh +- e_sh (body_ref.scale_shift) it lies between the extremes of the four corners;
    each end moves out by u |z| for the fp32 rounding of the fma where the compiler rounds twice (v_pk_fma_f32 + convert
    instead of v_fma_mixlo_f16: DESIGN.md) and the float64 roundoff of forming z here.  Rounding to fp16 and the LeakyReLU form
    (slope >= 0) are monotone: lo <= device <= hi.  open = the number of elements whose bracket holds more than one value."""
    x = np.asarray(x, np.float64)
    sc, sh, e_sc, e_sh = (_ex(a, x.ndim) for a in scale_shift(x, norm[0], norm[1], eps=eps))
    zs = [x * (sc + a * e_sc) + (sh + b * e_sh) for a in (-1, 1) for b in (-1, 1)]
    z_lo, z_hi = np.minimum.reduce(zs), np.maximum.reduce(zs)
    z_lo, z_hi = z_lo - U32 * np.abs(z_lo), z_hi + U32 * np.abs(z_hi)
    v, lo, hi = (act16(h16(z), slope) for z in (x * sc + sh, z_lo, z_hi))
    return v, lo, hi, int((lo != hi).sum())


def _t(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype))


def _pos0(y):
    """-0 -> +0: the accumulators start at +0 or at the bias, and (+0) + (-0) = +0"""
    return y + 0.0


def fits_exact(a, w, bias=None):
    """True when every fp32 partial sum of the conv of the staged activations a [n, cin, ...] with the weights w [cout, cin,
    taps...] (or [cin, cout, taps...] of a transposed conv: pass w.swapaxes(0, 1)) and the bias is exact in ANY order:
    in units of the data's common power-of-two quantum q = min(quantum(a) quantum(w), quantum(bias)),
        sum |w a| + |bias| < 2^24 for every output.
    Checked through the bound max |a| * sum_taps |w[co]| + |bias[co]| (sufficient: a False can be pessimistic)."""
    a, w = np.asarray(a, np.float64), np.asarray(w, np.float64)
    b = np.zeros(w.shape[0]) if bias is None else np.asarray(bias, np.float32).astype(np.float64)
    q = min(quantum(a) * quantum(w), quantum(b)) if np.any(b) else quantum(a) * quantum(w)
    mag = np.abs(a).max() * np.abs(w).reshape(w.shape[0], -1).sum(1) + np.abs(b)
    return bool((mag / q < 2.0 ** 24).all())


def conv_exact(a, w, bias, k, stride, fast=False):
    """Conv3d (zero padding (k - 1) / 2) of the staged activations a [n, cin, D, H, W] -> (t, y16): the float64 result and
    f16(t) rounded straight from float64, zeros as +0.  fast: float32 arithmetic - exact too, and only allowed, when
    fits_exact holds (asserted)."""
    pad = [(i - 1) // 2 for i in k]
    if fast:
        assert fits_exact(a, w, bias)
    dt = np.float32 if fast else np.float64
    b = None if bias is None else _t(np.asarray(bias, np.float32), dt)
    t = F.conv3d(_t(a, dt), _t(w, dt), b, list(stride), pad).numpy().astype(np.float64)
    return t, _pos0(h16(t))


def tconv_exact(a, w, bias, stride, fast=False):
    """ConvTranspose3d (kernel = stride) of a [n, cin, D, H, W] with w [cin, cout, *stride] -> (t, y16) as conv_exact"""
    if fast:
        assert fits_exact(a, np.asarray(w).swapaxes(0, 1), bias)
    dt = np.float32 if fast else np.float64
    b = None if bias is None else _t(np.asarray(bias, np.float32), dt)
    t = F.conv_transpose3d(_t(a, dt), _t(w, dt), b, list(stride)).numpy().astype(np.float64)
    return t, _pos0(h16(t))


def stats_exact(y):
    """(sum y, sum y^2) per (item, channel) of the fp16-valued outputs y [n, c, ...], float64 [n, c, 2] (exact: the sums are
    integers below 2^53 in quantum units for every tensor a test holds)"""
    y = np.asarray(y, np.float64)
    flat = y.reshape(y.shape[0], y.shape[1], -1)
    return np.stack((flat.sum(2), (flat * flat).sum(2)), -1)


def stats_fit_exact(y):
    """True when sum_item y^2 < 2^24 in units of quantum(y)^2 for every (item, channel): then |sum y| is below 2^24 quanta as
    well and every fp32 partial of the epilogue (the dot2 chains, row16_sum, a persistent workgroup's chain over its tiles) is
    an exactly representable integer multiple, whatever the kernel's order."""
    y = np.asarray(y, np.float64)
    q = quantum(y)
    flat = y.reshape(y.shape[0], y.shape[1], -1) / q
    return bool(((flat * flat).sum(2) < 2.0 ** 24).all())


def craft_norm(x, S, H, eps=1e-5):
    """(gamma, beta) float32 [c] for which stats_finalize_kernel arrives at f16(scale) == S[c] and f16(shift) == H[c] on
    the raw tensor x [n, c, ...]; S, H fp16-exact targets per channel.  gamma = f32(S sqrt(var + eps)), beta = f32(H + mean
    scale) with scale the float64 value of the rounded gamma.  gamma and beta are per channel, the statistics per item: every
    item's channel must hold the same multiset of values (asserted through the sums)."""
    x = np.asarray(x, np.float64)
    S, H = np.asarray(S, np.float64), np.asarray(H, np.float64)
    assert (h16(S) == S).all() and (h16(H) == H).all()
    n, c = x.shape[:2]
    flat = x.reshape(n, c, -1)
    s1, s2 = flat.sum(2), (flat * flat).sum(2)
    assert (s1 == s1[:1]).all() and (s2 == s2[:1]).all(), 'items differ in their statistics'
    inv_count = float(np.float32(1) / np.float32(flat.shape[2]))
    mean = s1[0] * inv_count
    var = np.maximum(s2[0] * inv_count - mean * mean, 0)
    root = np.sqrt(var + float(np.float32(eps)))
    gamma = (S * root).astype(np.float32)
    beta = (H + mean * (gamma.astype(np.float64) / root)).astype(np.float32)
    return gamma, beta


def stem_window(vol, origin, flips, patch):
    """the patch window [C, *patch] the stem reads from the volume vol [C, X, Y, Z], mirrored along the flagged axes (the
    output is NOT mirrored back: the seg head un-mirrors)"""
    vol = np.asarray(vol)
    x = vol[(slice(None),) + tuple(slice(int(o), int(o) + int(p)) for o, p in zip(origin, patch))]
    assert x.shape[1:] == tuple(patch), 'the patch leaves the volume'
    for ax in range(3):
        if flips[ax]:
            x = np.flip(x, 1 + ax)
    return np.ascontiguousarray(x)


def stem_exact(vol, origin, flips, patch, w, bias, fast=False):
    """The stem on one patch of vol [C, X, Y, Z] -> (t, y16) [1, cout, *patch] as conv_exact: window, mirror, x and w rounded
    to fp16, zero padding at the patch border (conv_exact's)"""
    x = h16(stem_window(vol, origin, flips, patch))[None]
    w = np.asarray(w)
    return conv_exact(x, h16(w), bias, w.shape[2:], (1, 1, 1), fast=fast)


def stem_batch(vol, origins, flips, patch, w, bias, fast=False):
    """stem_exact over a batch: vol [C, X, Y, Z] (one volume) or [n, C, X, Y, Z] -> y16 [n, cout, *patch]"""
    vol = np.asarray(vol)
    return np.concatenate([stem_exact(vol if vol.ndim == 4 else vol[i], o, flips, patch, w, bias, fast)[1] for i, o in enumerate(origins)])


def fused_stem_staged(y16, norm, slope, margin=1.0):
    """what a FUSE_STEM consumer multiplies: stage16 of the stem's stored values -> (value, lo, hi, ambiguous)"""
    return stage16(y16, norm, slope, margin=margin)


def fused_tconv_staged(low, low_norm, low_slope, tw, tbias, stride, skip, skip_norm, skip_slope, margin=1.0, fast=False):
    """what a FUSE_TCONV consumer multiplies: concat(f16(tconv(stage16(low))), stage16(skip)) -> (value, ambiguous)"""
    a, _, _, amb = stage16(low, low_norm, low_slope, margin=margin)
    up = tconv_exact(a, tw, tbias, stride, fast=fast)[1]
    b, _, _, amb2 = stage16(skip, skip_norm, skip_slope, margin=margin)
    return np.concatenate((up, b), 1), amb + amb2
