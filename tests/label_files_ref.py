"""The numpy yardstick of the label-file tests: which voxels of a file are labels, restated from the rule in include/fnn.h
(``fnn_decode_labels``) without a line of fast_nnunet_amd/imageio.py.

The value judged for a voxel is the float32 the image decode gives it - ``np.float32(np.float64(v) * slope + inter)``, the
product and the sum each rounded to float64, the multiply skipped for slope 1 and the add for intercept 0; without scaling
the plain cast, and for an integer datatype the integer itself.  A voxel is a label when that value is integral and lies in
[0, 255] (1-byte maps) or [0, 65535] (2-byte maps).  Every other voxel is stored as 0 and raises exactly one flag, the first
that applies: NOT_INTEGRAL (also NaN and the infinities), NEGATIVE, TOO_LARGE.
"""
import numpy as np

NOT_INTEGRAL, NEGATIVE, TOO_LARGE = 1, 2, 4
TOP = {1: 255, 2: 65535}
OUT_DTYPE = {1: np.uint8, 2: np.uint16}
NIFTI_CODES = {2: 'u1', 256: 'i1', 4: 'i2', 512: 'u2', 8: 'i4', 768: 'u4', 16: 'f4', 64: 'f8'}


def judged_values(v, scale, slope=1.0, inter=0.0):
    """What is judged: int64 for an unscaled integer datatype (no floating point), else the image decode's float32."""
    v = np.asarray(v)
    if not scale:
        if v.dtype.kind in 'iu':
            return v.astype(np.int64)
        with np.errstate(over='ignore', invalid='ignore'):
            return v.astype(np.float32)
    d = v.astype(np.float64)
    if slope != 1:
        d = d * np.float64(slope)
    if inter != 0:
        d = d + np.float64(inter)
    with np.errstate(over='ignore', invalid='ignore'):
        return d.astype(np.float32)


def judge(v, scale, slope, inter, out_bytes):
    """-> (labels uint8 / uint16 of v's shape, the flags of all voxels OR-ed, the largest valid label or 0)."""
    j = judged_values(v, scale, slope, inter)
    flag = np.zeros(j.shape, np.int32)
    if j.dtype.kind == 'f':
        with np.errstate(invalid='ignore'):
            odd = ~np.isfinite(j) | (np.floor(j) != j)
    else:
        odd = np.zeros(j.shape, bool)
    flag[odd] = NOT_INTEGRAL
    with np.errstate(invalid='ignore'):
        flag[~odd & (j < 0)] = NEGATIVE
        flag[~odd & (j > TOP[out_bytes])] = TOO_LARGE
    labels = np.zeros(j.shape, OUT_DTYPE[out_bytes])
    good = flag == 0
    labels[good] = j[good].astype(np.int64).astype(OUT_DTYPE[out_bytes])
    flags = int(np.bitwise_or.reduce(flag.reshape(-1))) if flag.size else 0
    return labels, flags, int(labels.max()) if labels.size else 0


def file_labels(values_f32_or_int, out_bytes):
    """``judge`` for values that are already what is judged (nifti_ref.read's float32 array)."""
    return judge(values_f32_or_int, 0, 1.0, 0.0, out_bytes)
