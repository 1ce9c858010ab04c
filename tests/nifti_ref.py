"""Yardstick for the image I/O tests: a NIfTI-1 reader and writer written from the NIfTI-1 specification (nifti1.h) with
numpy, struct and gzip.  It shares no code with ``fast_nnunet_amd.imageio``: the header is one numpy structured dtype, the
file is read whole, the values are computed by numpy on the host.

``read(fname) -> (float32 [z, y, x], info)``: the values of nibabel's ``get_fdata()`` (float64 scaling) cast to float32 and
transposed the way the reference's ``NibabelIO.read_images`` returns them, with ``info`` = affine (sform > qform > base),
spacing (z, y, x), sform, qform, the header record.
"""
import gzip

import numpy as np

FIELDS = [('sizeof_hdr', 'i4'), ('data_type', 'S10'), ('db_name', 'S18'), ('extents', 'i4'), ('session_error', 'i2'),
          ('regular', 'S1'), ('dim_info', 'u1'), ('dim', 'i2', (8,)), ('intent_p1', 'f4'), ('intent_p2', 'f4'),
          ('intent_p3', 'f4'), ('intent_code', 'i2'), ('datatype', 'i2'), ('bitpix', 'i2'), ('slice_start', 'i2'),
          ('pixdim', 'f4', (8,)), ('vox_offset', 'f4'), ('scl_slope', 'f4'), ('scl_inter', 'f4'), ('slice_end', 'i2'),
          ('slice_code', 'u1'), ('xyzt_units', 'u1'), ('cal_max', 'f4'), ('cal_min', 'f4'), ('slice_duration', 'f4'),
          ('toffset', 'f4'), ('glmax', 'i4'), ('glmin', 'i4'), ('descrip', 'S80'), ('aux_file', 'S24'),
          ('qform_code', 'i2'), ('sform_code', 'i2'), ('quatern_b', 'f4'), ('quatern_c', 'f4'), ('quatern_d', 'f4'),
          ('qoffset_x', 'f4'), ('qoffset_y', 'f4'), ('qoffset_z', 'f4'), ('srow_x', 'f4', (4,)), ('srow_y', 'f4', (4,)),
          ('srow_z', 'f4', (4,)), ('intent_name', 'S16'), ('magic', 'S4')]
HDR_LE = np.dtype(FIELDS).newbyteorder('<')
HDR_BE = np.dtype(FIELDS).newbyteorder('>')
assert HDR_LE.itemsize == 348
NUMPY_TYPES = {2: 'u1', 4: 'i2', 8: 'i4', 16: 'f4', 64: 'f8', 256: 'i1', 512: 'u2', 768: 'u4'}


def file_bytes(fname):
    if str(fname).endswith('.gz'):
        with gzip.open(fname, 'rb') as f:
            return f.read()
    with open(fname, 'rb') as f:
        return f.read()


def qform_affine(h):
    b, c, d = float(h['quatern_b']), float(h['quatern_c']), float(h['quatern_d'])
    a = np.sqrt(max(0.0, 1.0 - (b * b + c * c + d * d)))
    rot = np.array([[a * a + b * b - c * c - d * d, 2 * (b * c - a * d), 2 * (b * d + a * c)],
                    [2 * (b * c + a * d), a * a + c * c - b * b - d * d, 2 * (c * d - a * b)],
                    [2 * (b * d - a * c), 2 * (c * d + a * b), a * a + d * d - b * b - c * c]])
    qfac = -1.0 if float(h['pixdim'][0]) < 0 else 1.0
    out = np.eye(4)
    out[:3, 0] = rot[:, 0] * float(h['pixdim'][1])
    out[:3, 1] = rot[:, 1] * float(h['pixdim'][2])
    out[:3, 2] = rot[:, 2] * float(h['pixdim'][3]) * qfac
    out[:3, 3] = [float(h['qoffset_x']), float(h['qoffset_y']), float(h['qoffset_z'])]
    return out


def sform_affine(h):
    out = np.eye(4)
    out[0], out[1], out[2] = h['srow_x'], h['srow_y'], h['srow_z']
    return out


def base_affine(h):
    """nibabel's fallback: diag(-dx, dy, dz), the volume's centre voxel at the world origin."""
    n = np.array(h['dim'][1:4], dtype=np.float64)
    z = np.array(h['pixdim'][1:4], dtype=np.float64) * [-1, 1, 1]
    out = np.eye(4)
    out[[0, 1, 2], [0, 1, 2]] = z
    out[:3, 3] = -z * (n - 1) / 2
    return out


def read(fname):
    blob = file_bytes(fname)
    h = np.frombuffer(blob[:348], dtype=HDR_LE)[0]
    order = '<'
    if h['sizeof_hdr'] != 348:
        h = np.frombuffer(blob[:348], dtype=HDR_BE)[0]
        order = '>'
    assert h['sizeof_hdr'] == 348 and h['magic'] == b'n+1' and h['dim'][0] == 3
    nx, ny, nz = (int(i) for i in h['dim'][1:4])
    dt = np.dtype(NUMPY_TYPES[int(h['datatype'])]).newbyteorder(order)
    off = int(h['vox_offset'])
    vox = np.frombuffer(blob, dtype=dt, count=nx * ny * nz, offset=off).reshape(nz, ny, nx)
    slope, inter = np.float64(h['scl_slope']), np.float64(h['scl_inter'])
    if slope == 0 or not np.isfinite(slope):
        slope, inter = np.float64(1), np.float64(0)
    if slope == 1 and inter == 0:
        values = vox
    else:
        values = vox.astype(np.float64)
        if slope != 1:
            values = values * slope
        if inter != 0:
            values = values + inter
    with np.errstate(over='ignore', invalid='ignore'):
        values = values.astype(np.float32)
    info = {'header': h, 'sform': sform_affine(h), 'qform': qform_affine(h), 'shape': (nz, ny, nx),
            'spacing': [float(abs(h['pixdim'][3])), float(abs(h['pixdim'][2])), float(abs(h['pixdim'][1]))], 'order': order}
    info['affine'] = info['sform'] if h['sform_code'] > 0 else info['qform'] if h['qform_code'] > 0 else base_affine(h)
    return values, info


def properties(info):
    """The properties the reference's NibabelIO hands on for a file read with ``read``."""
    return {'spacing': list(info['spacing']), 'nibabel_stuff': {'original_affine': info['affine'].copy()}}


def write(fname, array_zyx, datatype, order='<', slope=1.0, inter=0.0, sform=None, sform_code=0, quatern=(0, 0, 0),
          qoffset=(0, 0, 0), qform_code=0, pixdim=(1, 1, 1, 1), vox_offset=352, bitpix=None, dim0=3, pad_tail=0):
    """One NIfTI-1 file with the given header fields (whatever they are: the refusal tests write wrong ones) and the
    array's values stored as ``datatype`` in byte order ``order``.  ``pixdim`` = (qfac, dx, dy, dz)."""
    dt = np.dtype(NUMPY_TYPES.get(datatype, 'u1')).newbyteorder(order)
    h = np.zeros((), dtype=HDR_LE if order == '<' else HDR_BE)
    nz, ny, nx = array_zyx.shape
    h['sizeof_hdr'] = 348
    h['dim'] = [dim0, nx, ny, nz, 1, 1, 1, 1]
    h['datatype'] = datatype
    h['bitpix'] = dt.itemsize * 8 if bitpix is None else bitpix
    h['pixdim'] = list(pixdim) + [1, 1, 1, 1]
    h['vox_offset'] = vox_offset
    h['scl_slope'], h['scl_inter'] = slope, inter
    h['qform_code'], h['sform_code'] = qform_code, sform_code
    h['quatern_b'], h['quatern_c'], h['quatern_d'] = quatern
    h['qoffset_x'], h['qoffset_y'], h['qoffset_z'] = qoffset
    if sform is not None:
        h['srow_x'], h['srow_y'], h['srow_z'] = sform[0], sform[1], sform[2]
    h['magic'] = b'n+1'
    with np.errstate(invalid='ignore'):
        body = np.ascontiguousarray(array_zyx.astype(dt)).tobytes()
    blob = h.tobytes() + b'\0' * (max(vox_offset, 348) - 348) + body + b'\0' * pad_tail
    opener = gzip.open if str(fname).endswith('.gz') else open
    with opener(fname, 'wb') as f:
        f.write(blob)
    return blob
