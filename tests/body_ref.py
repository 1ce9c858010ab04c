"""float64 restatement of the kernels between the convs (csrc/body.hip, head.hip: avgpool_kernel, combine_kernel,
combine_pool_kernel, the seg-head family, patch_acc_kernel, patch_input_kernel) that tests/test_gpu_body_ops.py compares the
device against, one op at a time.  Plain numpy, no device code.

Every function returns the float64 value `t` of the operation on the operands the kernel sees (fp16-rounded tensors, the
InstanceNorm scale / shift of stats_finalize_kernel) and a per-element bound on |device - t| that is the sum of the
roundings the kernel's arithmetic is stated to make, each one priced at the magnitude it rounds.  Nothing here is fitted
to what a device returned; a figure that had to be measured would be marked as such (there is none: see
HEAD_KSTEP_EXCESS).  tests/test_body_ref_cpu.py ties the values to oracle/unet.py in double precision.

Roundings counted (u = 2^-24, the unit roundoff of fp32):
  transform on load   v = fl32(fma(x, s, h))            u |v|, plus what the fp32 (s, h) themselves carry (scale_shift)
  LeakyReLU           v * slope where the slope is not 1  u |v slope|
  the add             fl32(ya + yb)                       u |ya + yb|
  pooling             fp32 sum of cnt terms, * fl32(1 / cnt)   (cnt - 1) u sum|y| + 2 u |sum| (the reciprocal and the product)
  store               one fp16 rounding                   half an fp16 ulp (2^-25 below 2^-14: subnormal spacing 2^-24)
"""
import numpy as np

# fp32 unit roundoff.  The bounds below are first-order sums k * u * magnitude; the factor (1 + 2^-12) covers the
# second-order terms of up to 2^11 compounded roundings (k u <= 2^-13 there), the largest count any op here reaches
# being the 161 of a 160-channel head, and the float64 roundoff of forming the reference itself (2^-53 per operation).
U32 = 2.0 ** -24 * (1 + 2.0 ** -12)
INT_MAX = 2 ** 31 - 1
# What v_mfma_f32_16x16x32_f16 adds to the any-order summation bound of head(): nothing.  The bound of head() is the
# derived (K + 1) u (sum |w x| + |bias|); on an MI355X the fp32 logits of seg_head_kernel (no store rounding in the way)
# used at most 0.17 of it over the committed cases of tests/test_gpu_body_ops.py whose operands are unambiguous
# (head_operand: spread 0), so no measured excess term is carried (contrast fp8_ref.MFMA_KSTEP_REL for the e4m3
# instruction).
HEAD_KSTEP_EXCESS = 0.0


def h16(a):
    """values rounded to fp16 once (round to nearest even), as float64: what the wrappers upload for a float32 operand, and
    what one fp16 rounding of an exact float64 result gives (straight from float64: a detour through float32 would round
    twice and land on the wrong side of a tie about once in 2^13 values)"""
    with np.errstate(over='ignore'):
        return np.asarray(a, np.float64).astype(np.float16).astype(np.float64)


def half_ulp16(mag):
    """half the spacing of fp16 numbers at magnitude `mag` (float64 array): the error of one round-to-nearest store.
    Normal range: 2^(floor(log2 mag) - 11); below 2^-14 the spacing is the subnormal 2^-24."""
    m = np.maximum(np.abs(np.asarray(mag, np.float64)), 2.0 ** -14)
    _, e = np.frexp(m)                                   # m = f * 2^e, f in [0.5, 1): floor(log2 m) = e - 1
    return np.ldexp(1.0, e - 1 - 11)


def store16(t, err):
    """bound on |fp16(t') - t| for a device value t' within err of t: err + half an ulp at the larger magnitude"""
    return err + half_ulp16(np.abs(t) + err)


def _ex(a, ndim):
    """[n, c] -> broadcastable over [n, c, ...]"""
    return np.asarray(a)[(slice(None), slice(None)) + (None,) * (ndim - 2)]


def scale_shift(x, gamma, beta, eps=1e-5, exact=False):
    """InstanceNorm of the fp16-valued raw tensor x [n, c, ...] as the per-(item, channel) affine y = x * sc + sh that
    stats_finalize_kernel hands to the consumers -> (sc, sh, e_sc, e_sh), float64 [n, c].
    The kernel works in double on exact sums with the wrapper's count reciprocal fl32(1 / voxels) and the fp32 eps, then
      rstd = fl32(1 / sqrt(var + eps)); sc = fl32(gamma * rstd); sh = fl32(beta - fl32(fl32(mean) * sc))
    sc carries two fp32 roundings: e_sc = 2 u |sc|.  The product fl32(mean) * sc carries those two, the rounding of the mean
    and its own (4 u |mean sc|), the subtraction one more of |beta| + |mean sc| (whether or not the compiler fuses product
    and subtraction: fusing removes a rounding): e_sh = u (5 |mean sc| + |beta|).
    exact = True: the mathematical InstanceNorm (count reciprocal 1 / voxels, eps as given), e_sc = e_sh = 0 - the form the
    CPU test compares with torch's double-precision InstanceNorm."""
    x = np.asarray(x, np.float64)
    n, c = x.shape[:2]
    flat = x.reshape(n, c, -1)
    inv_count = 1.0 / flat.shape[2] if exact else float(np.float32(1) / np.float32(flat.shape[2]))
    eps = float(eps) if exact else float(np.float32(eps))
    g = np.asarray(gamma, np.float32).astype(np.float64)[None] if not exact else np.asarray(gamma, np.float64)[None]
    b = np.asarray(beta, np.float32).astype(np.float64)[None] if not exact else np.asarray(beta, np.float64)[None]
    mean = flat.sum(2) * inv_count
    var = np.maximum((flat * flat).sum(2) * inv_count - mean * mean, 0)
    sc = g / np.sqrt(var + eps)
    sh = b - mean * sc
    if exact:
        return sc, sh, np.zeros_like(sc), np.zeros_like(sh)
    return sc, sh, 2 * U32 * np.abs(sc), U32 * (5 * np.abs(mean * sc) + np.abs(b))


def leaky(v, slope):
    return np.where(v > 0, v, v * slope)


def _leaky_err(y, e_in, slope):
    """LeakyReLU is Lipschitz with constant max(1, |slope|), so an input error passes through scaled by that at most (also
    when it moves the value across 0); the product with a slope other than 1 rounds once."""
    return max(1.0, abs(slope)) * e_in + (U32 * np.abs(y) if slope != 1.0 else 0.0)


def transform(x, ss=None, slope=1.0):
    """An operand as avgpool / combine load it (apply8): LeakyReLU(fl32(fma(x, sc, sh)), slope) of the fp16-valued x
    [n, c, ...]; ss = scale_shift(...) or None (identity: the value is x itself, no rounding) -> (y, e_y)."""
    x = np.asarray(x, np.float64)
    slope = float(np.float32(slope))
    if ss is None:
        v, e_v = x, np.zeros_like(x)
    else:
        sc, sh, e_sc, e_sh = (_ex(a, x.ndim) for a in ss)
        v = x * sc + sh
        e_v = np.abs(x) * e_sc + e_sh + U32 * np.abs(v)
    y = leaky(v, slope)
    return y, _leaky_err(y, e_v, slope)


def _blocks(y, stride):
    """[n, c, D, H, W] -> [n, c, D/s0, H/s1, W/s2, s0*s1*s2] (sizes truncated to whole blocks, like AvgPool3d)"""
    n, c, D, H, W = y.shape
    s0, s1, s2 = stride
    Do, Ho, Wo = D // s0, H // s1, W // s2
    y = y[:, :, :Do * s0, :Ho * s1, :Wo * s2].reshape(n, c, Do, s0, Ho, s1, Wo, s2)
    return y.transpose(0, 1, 2, 4, 6, 3, 5, 7).reshape(n, c, Do, Ho, Wo, s0 * s1 * s2)


def pool(y, e_y, stride):
    """AvgPool3d(stride, stride) of values y known to within e_y -> (t, bound before the store).  The kernels add the cnt
    terms in fp32 one after the other ((cnt - 1) roundings, each of a partial sum of magnitude <= sum |y|), multiply by
    fl32(1 / cnt) (one rounding of the reciprocal, exact for a power of two, and one of the product)."""
    yb, eb = _blocks(np.asarray(y, np.float64), stride), _blocks(np.broadcast_to(e_y, np.shape(y)).astype(np.float64), stride)
    cnt = yb.shape[-1]
    mag = np.abs(yb).sum(-1)
    return yb.sum(-1) / cnt, (eb.sum(-1) + (cnt + 1) * U32 * mag) / cnt


def avgpool(x, stride, ss=None, slope=1.0):
    """avgpool_kernel -> (t, bound): fp16(mean over the block of transform(x))"""
    t, e = pool(*transform(x, ss, slope), stride)
    return t, store16(t, e)


def combine(a, b, slope, ss_a=None, slope_a=1.0, ss_b=None, slope_b=1.0):
    """combine_kernel / the block output of combine_pool_kernel -> (t, bound):
    fp16(LeakyReLU(fl32(transform(a) + transform(b)), slope))"""
    ya, ea = transform(a, ss_a, slope_a)
    yb, eb = transform(b, ss_b, slope_b)
    s = ya + yb
    e_s = ea + eb + U32 * np.abs(s)
    slope = float(np.float32(slope))
    t = leaky(s, slope)
    return t, store16(t, _leaky_err(t, e_s, slope))


def pooled_of_output(y16, stride):
    """The pooled tensor of combine_pool_kernel from the block output y16 the SAME launch stored (fp16 values, checked
    against combine() on its own): the mean of the fp16-rounded outputs, fp32 sum, one fp16 rounding -> (t, bound)."""
    t, e = pool(np.asarray(y16, np.float64), 0.0, stride)
    return t, store16(t, e)


# ---- seg head ----------------------------------------------------------------------------------------------------------
def head_operand(x, ss=None, slope=1.0):
    """The B operand the seg-head kernels form from the raw fp16 features x [n, c, ...] (fnn_norm8 and the LeakyReLU
    behind it, csrc/fnn_device.h: the engine's normalise-on-load in packed fp16): scale and shift rounded to fp16, one fused
    multiply-add rounded to fp16, then max(o, fp16(o * fp16(slope))).  Products and sums of fp16 values are exact in
    float64, so for given fp16 (scale, shift) this is the operand itself, not an estimate -> (xop, spread).
    The fp16 rounding of a scale or shift can depend on the last bits of its fp32 value (scale_shift: known to within e_sc,
    e_sh) when that value sits on an fp16 rounding boundary - about one (item, channel) in two thousand.  The operand is
    monotone in both, so the device's lies between the extremes over the roundings of both ends of each interval:
    spread = max - min over those four (0 wherever the roundings agree, i.e. almost everywhere), which head() prices
    at |w| * spread.  ss = None: the identity affine (scale 1, shift 0), spread 0; the LeakyReLU still applies."""
    x = np.asarray(x, np.float64)
    sl = h16(slope)
    act = lambda o: np.maximum(o, h16(o * sl))
    if ss is None:
        return act(x), np.zeros_like(x)
    sc, sh, e_sc, e_sh = ss
    op = lambda s, h: act(h16(x * _ex(h16(s), x.ndim) + _ex(h16(h), x.ndim)))
    cands = [op(s, h) for s in (sc - e_sc, sc + e_sc) for h in (sh - e_sh, sh + e_sh)]
    return op(sc, sh), np.maximum.reduce(cands) - np.minimum.reduce(cands)


def head(xop, w, bias, spread=None):
    """1x1x1 conv of one item: xop [c, P] (head_operand), w [heads, c] fp16 values, bias [heads] fp32 values -> (t, bound),
    [heads, P].  Products of two fp16 values are exact in fp32; the MFMA chain adds K = 32 * ceil(c_pad / 32) of them
    (zeros included) and the bias in fp32 in an order nobody documents: the any-order bound (K + 1) u (sum |w x| + |bias|).
    The result stays in fp32 (no store rounding here).  spread: head_operand's, [c, P]."""
    xop, w = np.asarray(xop, np.float64), np.asarray(w, np.float64)
    b = np.zeros(w.shape[0]) if bias is None else np.asarray(bias, np.float32).astype(np.float64)
    c = w.shape[1]
    K = 32 * (((c + 15) // 16 * 16 + 31) // 32)
    t = w @ xop + b[:, None]
    mag = np.abs(w) @ np.abs(xop) + np.abs(b)[:, None]
    e = ((K + 1) * U32 + HEAD_KSTEP_EXCESS) * mag
    return t, (e if spread is None else e + np.abs(w) @ spread)


def unflip(t, patch, flips):
    """[heads, P] in the (mirrored) network's voxel order -> [heads, P] in patch space"""
    a = np.asarray(t).reshape(t.shape[0], *patch)
    for ax in range(3):
        if flips[ax]:
            a = np.flip(a, 1 + ax)
    return np.ascontiguousarray(a).reshape(t.shape[0], -1)


def first_mask(patch, first):
    """[PD, PH, PW] bool: the voxels HeadParams::fx / fy / fz declare untouched by any earlier patch"""
    d, h, w = np.meshgrid(*[np.arange(p) for p in patch], indexing='ij')
    return (d >= first[0]) & (h >= first[1]) & (w >= first[2])


def accumulate(a_old, t, e_t, g, fp32, first=None):
    """Accumulator channels of the heads after one patch: a_old [heads, P] (the accumulator's values, float64), t / e_t the
    logits and their bound [heads, P], g [P] the fp16 weights as float64, first [P] bool or None -> (value, bound).
      c = fl32(t * g), never fused into the add; s = fl32(a + c) with a = 0 on first-visit voxels; fp16 accumulators round s
      once more to fp16."""
    a = np.where(first[None], 0.0, a_old) if first is not None else np.asarray(a_old, np.float64)
    c = t * g[None]
    e_c = e_t * g[None] + U32 * np.abs(c)
    s = a + c
    e = e_c + U32 * np.abs(s)
    return s, (e if fp32 else store16(s, e))


def weight_channel(a_old, g_bits, fp32, first=None):
    """Channel `heads` after one patch, exactly: fl32(a + g) for fp32 accumulators, fp16(fl32(a + g)) for fp16 ones
    (a = 0 on first-visit voxels).  a_old [P] in the accumulator's dtype, g_bits [P] uint16 -> the accumulator's dtype."""
    g = np.asarray(g_bits, np.uint16).view(np.float16).astype(np.float32)
    a = np.asarray(a_old).astype(np.float32)
    if first is not None:
        a = np.where(first, np.float32(0), a)
    s = (a + g).astype(np.float32)
    return s if fp32 else s.astype(np.float16)


def patch_mean(patch_buf, n_div):
    """patch_acc_kernel's logit: fl32(patch_buf / n_div) -> (t, bound) (exact for a power of two; one rounding otherwise)"""
    t = np.asarray(patch_buf, np.float64) / n_div
    return t, U32 * np.abs(t)


def patch_input(vol, origins, patch, cpad, flips):
    """patch_input_kernel, exactly: fp16(vol[window]) mirrored by flips, zeros in the padding channels -> uint16 bits
    [n, cpad, PD, PH, PW].  vol [C, X, Y, Z] (every item reads it) or [n, C, X, Y, Z]."""
    vol = np.asarray(vol, np.float32)
    origins = np.asarray(origins).reshape(-1, 3)
    out = np.zeros((origins.shape[0], cpad, *patch), np.float16)
    for i, o in enumerate(origins):
        v = vol if vol.ndim == 4 else vol[i]
        w = v[:, o[0]:o[0] + patch[0], o[1]:o[1] + patch[1], o[2]:o[2] + patch[2]]
        for ax in range(3):
            if flips[ax]:
                w = np.flip(w, 1 + ax)
        with np.errstate(over='ignore'):
            out[i, :v.shape[0]] = w.astype(np.float16)
    return out.view(np.uint16)
