"""float64 restatement of the e4m3 conv path (conv3d_zr8_kernel on the weights conv_pack_weights packs) that
the fp8 op tests compare the device against.  Every quantisation goes through torch's float8_e4m3fn (OCP e4m3, round to
nearest even; clamped to +-448 first, as the kernel and the packer saturate there)."""
import numpy as np
import torch
import torch.nn.functional as F

ACT_MULT = 8.0                  # FNN_FP8_ACT_MULT
E4M3_MAX = 448.0
F32_EPS = 2.0 ** -24            # unit roundoff of fp32
# v_mfma_f32_16x16x32_fp8_fp8 does not return the fp32-rounded sum of its 32 products: on an MI355X its result was measured
# off by up to 2^-13.4 of the largest product magnitude the output's receptive field holds, per k-step (2^-12.7 over a whole
# 3x3x3 conv; no documented figure).  The bound takes 2^-12 of it per k-step.
MFMA_KSTEP_REL = 2.0 ** -12


def e4m3(v):
    """float32 values -> the nearest OCP e4m3 value after the clamp to +-448, as float64"""
    v = np.clip(np.asarray(v, np.float32), -E4M3_MAX, E4M3_MAX)
    return torch.from_numpy(np.ascontiguousarray(v)).to(torch.float8_e4m3fn).double().numpy()


def quantise_weights(w):
    """conv_pack_weights' e4m3 encoding.  w [cout, cin, kd, kh, kw] float32 -> (wq, oscale): wq the e4m3 weights (float64),
    oscale [cout] = f32(ws / 8) with ws = f32(max |w| / 448) per cout and wq = e4m3(f32(w * f32(1 / ws))).  A cout whose
    max |w| is 0, or so small that 1 / ws is not finite, has zero weights and ws = 1."""
    w = np.asarray(w, np.float32)
    cout = w.shape[0]
    mx = np.abs(w.reshape(cout, -1)).max(1).astype(np.float32)
    with np.errstate(divide='ignore', over='ignore', invalid='ignore'):
        ws = (mx / np.float32(E4M3_MAX)).astype(np.float32)
        inv = (np.float32(1) / ws).astype(np.float32)
    zero = ~(mx > 0) | ~np.isfinite(inv)
    ws = np.where(zero, np.float32(1), ws).astype(np.float32)
    inv = np.where(zero, np.float32(0), inv).astype(np.float32)
    v = (w * inv.reshape(-1, *([1] * (w.ndim - 1)))).astype(np.float32)
    return e4m3(v), (ws / np.float32(ACT_MULT)).astype(np.float32).astype(np.float64)


def norm_scale_shift(x, gamma, beta, eps=1e-5):
    """The (scale, shift) per (item, channel) that fnn_op_conv3d's InstanceNorm on load uses, in float64: statistics of the
    fp16-valued x [n, c, ...] with the wrapper's count reciprocal f32(1 / voxels) -> [n, c] arrays.  The kernel's own fp32
    values (stats_finalize_kernel) differ from these by a few fp32 ulps: act_bracket covers that."""
    x = np.asarray(x, np.float64)
    n, c = x.shape[:2]
    flat = x.reshape(n, c, -1)
    inv_count = float(np.float32(1) / np.float32(flat.shape[2]))
    mean = flat.sum(2) * inv_count
    var = np.maximum((flat * flat).sum(2) * inv_count - mean * mean, 0)
    rstd = 1.0 / np.sqrt(var + float(np.float32(eps)))
    sc = np.asarray(gamma, np.float32).astype(np.float64)[None] * rstd
    sh = np.asarray(beta, np.float32).astype(np.float64)[None] - mean * sc
    return sc, sh, np.abs(mean * sc) + np.abs(np.asarray(beta, np.float32).astype(np.float64))[None]


def act_bracket(x, norm=None, slope=1.0, ulps=8):
    """The staging quantiser q = e4m3(clamp(LeakyReLU(8 * (x * sc + sh)), +-448)) of conv3d_zr8_kernel for x [n, c, ...]
    (fp16 values).  norm = None: sc = 1, sh = 0, and 8 x is exact in fp32 - (q, q, q).  norm = (gamma, beta): the kernel's
    fp32 value lies within `ulps` fp32 ulps of |8 x sc| + |8 sh| (+ the shift's own terms) of the float64 one; both ends of
    that interval are quantised -> (q, q_lo, q_hi), float64 arrays.  LeakyReLU multiplies by the fp32 slope."""
    x = np.asarray(x, np.float64)
    if norm is None:
        q = e4m3((x * ACT_MULT).astype(np.float32))
        return q, q, q
    sc, sh, terms = norm_scale_shift(x, *norm)
    ex = (slice(None), slice(None)) + (None,) * (x.ndim - 2)
    v = ACT_MULT * (x * sc[ex] + sh[ex])
    d = ulps * F32_EPS * ACT_MULT * (np.abs(x * sc[ex]) + np.abs(sh[ex]) + terms[ex])
    s = float(np.float32(slope))
    lrelu = lambda t: np.where(t >= 0, t, t * s)
    lo, mid, hi = lrelu(v - d), lrelu(v), lrelu(v + d)
    lo, hi = lo - 2 * F32_EPS * np.abs(lo), hi + 2 * F32_EPS * np.abs(hi)       # the fp32 product v * slope
    # rounding to fp32 is monotonic: f32(lo) <= the kernel's fp32 value <= f32(hi); so are the clamp and the e4m3 rounding
    return e4m3(mid.astype(np.float32)), e4m3(lo.astype(np.float32)), e4m3(hi.astype(np.float32))


def conv_e4m3(q, q_lo, q_hi, w, bias, chunks, pad=(1, 1, 1)):
    """conv3d_zr8_kernel's output for the staged activations (act_bracket, sources concatenated along channels) and the
    float32 weights w -> (y, tol, uncertain): y = fp16(acc * oscale + bias) as float64 with acc the float64 conv of the
    e4m3 operands (zero padding), tol per output = one fp16 ulp of y + the fp32 accumulation order (m = 15 k-steps per
    16-channel chunk, plus the scale and bias roundings) + MFMA_KSTEP_REL per k-step of the largest product |q| |wq| in the
    receptive field (the matrix core's own sum) + oscale * conv(|q_hi - q_lo|, |wq|), uncertain = the fraction of activations
    whose bracket holds more than one e4m3 value.  chunks: the layer's 16-channel chunks (sources padded apart)."""
    wq, oscale = quantise_weights(w)
    cout = wq.shape[0]
    b = np.zeros(cout) if bias is None else np.asarray(bias, np.float32).astype(np.float64)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float64))
    conv = lambda a, ww: F.conv3d(t(a), t(ww), None, 1, list(pad)).numpy()
    ex = (None, slice(None), None, None, None)
    acc = conv(q, wq)
    y = acc * oscale[ex] + b[ex]
    y16 = y.astype(np.float16).astype(np.float64)
    m = 15 * chunks + 2
    tol = np.spacing(np.abs(y16).astype(np.float16)).astype(np.float64)
    tol = tol + m * F32_EPS * oscale[ex] * conv(np.abs(q), np.abs(wq)) + 2 * F32_EPS * np.abs(b)[ex]
    qmax = F.max_pool3d(t(np.maximum(np.abs(q_lo), np.abs(q_hi)).max(1, keepdims=True)), 3, 1, list(pad)).numpy()
    tol = tol + 15 * chunks * MFMA_KSTEP_REL * oscale[ex] * qmax * np.abs(wq).reshape(cout, -1).max(1)[ex]
    uncertain = float((q_hi != q_lo).mean())
    if uncertain:
        tol = tol + oscale[ex] * conv(np.abs(q_hi - q_lo), np.abs(wq))
    return y16, tol, uncertain
