"""Image files in and out: a single-file NIfTI-1 reader and writer whose voxels are decoded on the device.

Restates, with the reference's method names and property keys, what its ``NibabelIO`` and ``SimpleITKIO`` classes
(imageio/nibabel_reader_writer.py:26-98, imageio/simpleitk_reader_writer.py:23-129) do for ``.nii`` / ``.nii.gz`` files,
without nibabel or SimpleITK: the header is parsed with ``struct``, ``.gz`` files are inflated with ``zlib`` and the
voxel bytes go to the device as they lie in the file, where ``fnn_decode_voxels`` (csrc/imageio.hip) turns them into the
float32 ``[C, z, y, x]`` tensor ``DevicePreprocessor.run_case_npy`` takes - half the upload of an int16 CT, a quarter for
uint8, and no host cast.

* array order: the reference's ``(z, y, x)``, which is the file's own memory order (x fastest): no transpose;
* values: nibabel's ``get_fdata()`` (float64 scaling, ``get_slope_inter`` rules) cast to float32;
* ``properties``: ``'spacing'`` (reversed ``abs(pixdim[1:4])``), ``'nibabel_stuff': {'original_affine'}`` (sform, else
  qform, else the base affine) and ``'sitk_stuff'`` (the same geometry in ITK's LPS convention - restated from published
  behaviour and not pinned against SimpleITK);
* ``write_seg``: the header ``nibabel.Nifti1Image(seg, affine)`` saves (pinned byte for byte by the reference's output
  fixture), gzip level 1.

``NiftiReorientIO`` is the reference's ``NibabelIOWithReorient`` (imageio/nibabel_reader_writer.py:101-190) on top of it:
images brought to RAS+ behind the decode and labels back to the file's frame before their download, each by one
``fnn_reorient`` pass (csrc/reorient.hip); nibabel's orientation rules are restated below, unpinned against nibabel.

``NiftiIO.compress_labels`` is the opt-in write route that never downloads the label map: ``fnn_deflate_labels``
(csrc/deflate.hip) turns the device labels into a deflate fragment, and ``write_seg`` only puts the gzip member together
around it (``DeviceCompressedLabels``, ``compressed_label_file_bytes``).  ``NiftiIO.compress_label_masks`` does the same for
the per-label mask files of ``jhu.JHUPredictor``: all masks of a map in one pass (csrc/deflate_masks.hip).

``NiftiIO.read_label_map`` reads a label file as labels: ``fnn_decode_labels`` (csrc/imageio.hip) turns the file's voxel
bytes into the uint8 / uint16 map the counting, labelling and compressing kernels take, and reports what is no label - a
file with such a voxel is refused (the reference would carry the voxel along as a value that equals no label).  The folder
front-ends (``evaluation.compute_metrics_on_folder``, ``postprocessing.apply_postprocessing_to_folder``, ...) read with it.

``NiftiIO(inflate_on_device=True)`` is the opt-in read route for exactly those files: ``StagedCase.fill`` stages the
compressed file as it is when ``chunked_layout`` recognises it, and ``decode_label_maps`` lets ``fnn_inflate_segments``
(csrc/inflate.hip) inflate it on the device, certified by the call's status and the gzip trailer's CRC-32.  Files written by
zlib (references, scanner images), image files and everything the device refuses are inflated by zlib on the host, as ever.
``fnn_inflate_segments`` refuses dynamic-Huffman blocks, so a file written with ``compress_on_device='dynamic'`` falls back;
``NiftiIO(inflate_on_device='dynamic')`` takes ``fnn_inflate_segments_dyn`` (csrc/inflate_dyn.hip) instead, which decodes
them and serves the files of both encoders.  ``NiftiIO(inflate_on_device='any')`` does that and stages every other
single-member ``.nii.gz`` label file too - what zlib, nibabel, SimpleITK or nnU-Net wrote (``stream_layout``) - for
``fnn_inflate_stream`` (csrc/inflate_any.hip), which inflates one deflate stream speculatively from every bit position at which a
dynamic block may begin; certified in the same way, with the same fallback.  On label maps, which zlib cuts into few blocks,
that route is slower than zlib on the host (profiles/r35_inflate_any.txt): it is an opt-in for streams of many blocks.

The header is untrusted: every length is checked against the file before anything is uploaded or launched.
"""
from __future__ import annotations

import gzip
import os
import struct
import warnings
import zlib
from typing import List, Optional, Sequence, Tuple, Union

import numpy as np

from . import capi

# NIfTI datatype code -> (numpy dtype character, bytes per voxel); what fnn_decode_voxels serves
DATATYPES = {2: ('u1', 1), 256: ('i1', 1), 4: ('i2', 2), 512: ('u2', 2), 8: ('i4', 4), 768: ('u4', 4), 16: ('f4', 4),
             64: ('f8', 8)}
_OTHER_DATATYPES = {1: 'binary', 32: 'complex64', 128: 'RGB24', 1024: 'int64', 1280: 'uint64', 1536: 'float128',
                    1792: 'complex128', 2048: 'complex256', 2304: 'RGBA32'}
SUPPORTED_FILE_ENDINGS = ('.nii', '.nii.gz')
_OTHER_FILE_ENDINGS = ('.hdr', '.img', '.img.gz', '.hdr.gz', '.nrrd', '.mha', '.mhd', '.gipl', '.tif', '.tiff', '.png', '.bmp')
HEADER_BYTES = 348
MIN_VOX_OFFSET = 352


class NiftiHeader:
    """The fields of a NIfTI-1 header this engine reads, checked (``fname`` only names the file in messages)."""

    def __init__(self, head: bytes, fname: str = '<bytes>'):
        def bad(msg):
            return RuntimeError(f'{fname}: {msg}')

        if len(head) < HEADER_BYTES + 4:
            raise bad(f'{len(head)} bytes are no NIfTI-1 header (352 expected)')
        size_le, = struct.unpack_from('<i', head, 0)
        size_be, = struct.unpack_from('>i', head, 0)
        if size_le == HEADER_BYTES:
            e = '<'
        elif size_be == HEADER_BYTES:
            e = '>'
        elif 540 in (size_le, size_be):
            raise NotImplementedError(f'{fname}: NIfTI-2 files are not read (single-file NIfTI-1 only)')
        else:
            raise bad(f'sizeof_hdr is {size_le}, not 348 in either byte order: no NIfTI-1 file')
        magic = bytes(head[344:348])
        if magic == b'ni1\0':
            raise NotImplementedError(f'{fname}: .hdr / .img pairs (magic "ni1") are not read (single-file NIfTI-1 only)')
        if magic != b'n+1\0':
            raise bad(f'magic {magic!r} is not "n+1"')
        self.endian = e
        self.byteswap = e == '>'
        dim = struct.unpack_from(e + '8h', head, 40)
        if dim[0] != 3:
            raise bad(f'dim[0] = {dim[0]}: only 3-D images are read (2-D and 4-D files are not)')
        if min(dim[1:4]) < 1:
            raise bad(f'extents {dim[1:4]} must be positive')
        self.shape_xyz = tuple(int(i) for i in dim[1:4])
        self.datatype, self.bitpix = (int(i) for i in struct.unpack_from(e + '2h', head, 70))
        if self.datatype not in DATATYPES:
            raise NotImplementedError(f'{fname}: NIfTI datatype {self.datatype} '
                                      f'({_OTHER_DATATYPES.get(self.datatype, "unknown")}) is not read')
        self.dtype_char, self.bytes_per_voxel = DATATYPES[self.datatype]
        if self.bitpix != 8 * self.bytes_per_voxel:
            raise bad(f'datatype {self.datatype} has {8 * self.bytes_per_voxel} bits per voxel, bitpix says {self.bitpix}')
        self.pixdim = np.array(struct.unpack_from(e + '8f', head, 76), dtype=np.float32)
        vox_offset, slope, inter = struct.unpack_from(e + '3f', head, 108)
        if not np.isfinite(vox_offset) or vox_offset < MIN_VOX_OFFSET or vox_offset != int(vox_offset):
            raise bad(f'vox_offset {vox_offset} (a whole number >= 352 expected)')
        self.vox_offset = int(vox_offset)
        self.n_vox = self.shape_xyz[0] * self.shape_xyz[1] * self.shape_xyz[2]
        self.n_bytes = self.n_vox * self.bytes_per_voxel
        # nibabel's get_slope_inter: slope 0 / non-finite = no scaling; a valid slope with a non-finite intercept is an error
        slope, inter = float(np.float32(slope)), float(np.float32(inter))
        if slope == 0 or not np.isfinite(slope):
            slope, inter = 1.0, 0.0
        elif not np.isfinite(inter):
            raise bad('valid scl_slope but invalid scl_inter')
        self.slope, self.inter = slope, inter
        self.scale = not (slope == 1.0 and inter == 0.0)
        self.qform_code, self.sform_code = (int(i) for i in struct.unpack_from(e + '2h', head, 252))
        self.quatern = np.array(struct.unpack_from(e + '6f', head, 256), dtype=np.float32)
        self.srow = np.array(struct.unpack_from(e + '12f', head, 280), dtype=np.float32).reshape(3, 4)
        self.spacing = [float(abs(self.pixdim[3])), float(abs(self.pixdim[2])), float(abs(self.pixdim[1]))]
        self.affine = self._best_affine()

    @property
    def shape(self) -> Tuple[int, int, int]:
        """(z, y, x): the array order of the reference."""
        return self.shape_xyz[::-1]

    def _best_affine(self) -> np.ndarray:
        a = np.eye(4, dtype=np.float64)
        if self.sform_code > 0:
            a[:3] = self.srow.astype(np.float64)
            return a
        zooms = self.pixdim[1:4].astype(np.float64)
        if self.qform_code > 0:
            b, c, d = (float(v) for v in self.quatern[:3])
            w2 = 1.0 - (b * b + c * c + d * d)
            if w2 < 0:                               # NIfTI-1: a = 0 and (b, c, d) normalised
                n = (b * b + c * c + d * d) ** 0.5
                b, c, d, aq = b / n, c / n, d / n, 0.0
            else:
                aq = w2 ** 0.5
            r = np.array([[aq * aq + b * b - c * c - d * d, 2 * b * c - 2 * aq * d, 2 * b * d + 2 * aq * c],
                          [2 * b * c + 2 * aq * d, aq * aq + c * c - b * b - d * d, 2 * c * d - 2 * aq * b],
                          [2 * b * d - 2 * aq * c, 2 * c * d + 2 * aq * b, aq * aq + d * d - c * c - b * b]])
            qfac = -1.0 if self.pixdim[0] < 0 else 1.0
            a[:3, :3] = r * (zooms * np.array([1.0, 1.0, qfac]))[None]
            a[:3, 3] = self.quatern[3:].astype(np.float64)
            return a
        # neither form: nibabel's base affine - the zooms on the diagonal (x flipped, its Analyze default), the centre
        # voxel at the origin
        zooms = zooms * np.array([-1.0, 1.0, 1.0])
        a[:3, :3] = np.diag(zooms)
        a[:3, 3] = -(np.array(self.shape_xyz, dtype=np.float64) - 1) / 2.0 * zooms
        return a


def sitk_stuff_from_affine(affine: np.ndarray) -> dict:
    """A RAS voxel-to-world affine as ITK states the geometry (LPS): spacing and origin in (x, y, z) order, direction the
    row-major 3x3 cosines."""
    lps = np.diag([-1.0, -1.0, 1.0, 1.0]) @ np.asarray(affine, dtype=np.float64)
    spacing = np.sqrt((lps[:3, :3] ** 2).sum(0))
    safe = np.where(spacing > 0, spacing, 1.0)
    direction = lps[:3, :3] / safe[None]
    return {'spacing': tuple(float(i) for i in spacing), 'origin': tuple(float(i) for i in lps[:3, 3]),
            'direction': tuple(float(i) for i in direction.reshape(-1))}


def affine_from_sitk_stuff(stuff: dict) -> np.ndarray:
    lps = np.eye(4, dtype=np.float64)
    lps[:3, :3] = np.asarray(stuff['direction'], dtype=np.float64).reshape(3, 3) * np.asarray(stuff['spacing'], dtype=np.float64)[None]
    lps[:3, 3] = np.asarray(stuff['origin'], dtype=np.float64)
    return np.diag([-1.0, -1.0, 1.0, 1.0]) @ lps


def _check_ending(fname: str) -> bool:
    """-> gzipped?  Raises NotImplementedError for every format but single-file NIfTI."""
    low = str(fname).lower()
    if low.endswith('.nii.gz'):
        return True
    if low.endswith('.nii'):
        return False
    for end in _OTHER_FILE_ENDINGS:
        if low.endswith(end):
            raise NotImplementedError(f'{fname}: {end} files are not read (this engine reads .nii and .nii.gz)')
    raise NotImplementedError(f'{fname}: unknown file ending (this engine reads .nii and .nii.gz)')


class _FileStream:
    """Sequential reads of a file's (inflated) bytes."""

    def __init__(self, fname: str):
        self.fname = fname
        gz = _check_ending(fname)                    # (before the file is touched: another format is refused by its name)
        self.f = open(fname, 'rb')
        self.z = zlib.decompressobj(wbits=31) if gz else None
        self.pending = b''

    def close(self):
        self.f.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _more(self) -> bytes:
        """The next piece of (inflated) bytes, b'' at the end (of the file, or of the gzip member)."""
        if self.z is None:
            return self.f.read(1 << 20)
        while not self.z.eof:
            raw = self.z.unconsumed_tail or self.f.read(1 << 20)
            if not raw:
                return b''
            out = self.z.decompress(raw, 1 << 22)
            if out:
                return out
        return b''

    def readinto(self, dst: memoryview) -> int:
        """Fills dst as far as the file reaches; -> bytes written."""
        n = 0
        try:
            while n < len(dst):
                if not self.pending:
                    self.pending = self._more()
                    if not self.pending:
                        break
                take = min(len(self.pending), len(dst) - n)
                dst[n:n + take] = self.pending[:take]
                self.pending = self.pending[take:]
                n += take
        except zlib.error as err:
            raise RuntimeError(f'{self.fname}: corrupt gzip stream ({err})') from None
        return n

    def read(self, n: int) -> bytes:
        buf = bytearray(n)
        return bytes(buf[:self.readinto(memoryview(buf))])

    def skip(self, n: int) -> int:
        done = 0
        scratch = memoryview(bytearray(min(n, 1 << 16))) if n else None
        while done < n:
            got = self.readinto(scratch[:min(len(scratch), n - done)])
            if not got:
                break
            done += got
        return done


def read_header(fname: str) -> NiftiHeader:
    with _FileStream(fname) as s:
        return NiftiHeader(s.read(MIN_VOX_OFFSET), fname)


def read_voxel_bytes(fname: str, hdr: NiftiHeader, dst: np.ndarray) -> None:
    """The file's ``hdr.n_bytes`` voxel bytes into ``dst`` (uint8, at least that long): pure host work, which is what the
    reader thread of ``predict_from_files`` runs.  RuntimeError when the file ends before its header says it should."""
    view = memoryview(dst).cast('B')[:hdr.n_bytes]
    with _FileStream(fname) as s:
        if s.skip(hdr.vox_offset) != hdr.vox_offset or s.readinto(view) != hdr.n_bytes:
            raise RuntimeError(f'{fname}: the file ends before vox_offset {hdr.vox_offset} + {hdr.n_vox} voxels of '
                               f'{hdr.bytes_per_voxel} bytes (truncated?)')


def check_case(fnames: Sequence[str], hdrs: Sequence[NiftiHeader]) -> None:
    """The files of one case: equal shapes and spacings (RuntimeError), equal affines (a warning) - as the reference."""
    if any(h.shape != hdrs[0].shape for h in hdrs):
        raise RuntimeError(f'Not all input images have the same shape! Shapes: {[h.shape for h in hdrs]} '
                           f'Image files: {list(fnames)}')
    if any(not np.array_equal(h.affine, hdrs[0].affine) for h in hdrs):
        warnings.warn(f'Not all input images have the same original_affines! Affines: {[h.affine for h in hdrs]} '
                      f'Image files: {list(fnames)}. It is up to you to decide whether that\'s a problem.')
    if any(h.spacing != hdrs[0].spacing for h in hdrs):
        raise RuntimeError(f'Not all input images have the same spacing_for_nnunet! This might be caused by them not '
                           f'having the same affine. spacings_for_nnunet: {[h.spacing for h in hdrs]} '
                           f'Image files: {list(fnames)}')


def case_properties(hdr: NiftiHeader) -> dict:
    return {'nibabel_stuff': {'original_affine': hdr.affine.copy()}, 'sitk_stuff': sitk_stuff_from_affine(hdr.affine),
            'spacing': list(hdr.spacing)}


def decode_on_host(hdr: NiftiHeader, raw: np.ndarray) -> np.ndarray:
    """numpy's statement of fnn_decode_voxels: float32 (z, y, x) from the file's voxel bytes."""
    v = np.frombuffer(memoryview(raw).cast('B')[:hdr.n_bytes], dtype=np.dtype(hdr.endian + hdr.dtype_char))
    if hdr.scale:
        v = v.astype(np.float64)
        if hdr.slope != 1.0:
            v = v * np.float64(hdr.slope)
        if hdr.inter != 0.0:
            v = v + np.float64(hdr.inter)
    with np.errstate(over='ignore', invalid='ignore'):
        return v.astype(np.float32).reshape(hdr.shape)


# ---------------------------------------------------------------------- label files
LABEL_FLAG_NOT_INTEGRAL, LABEL_FLAG_NEGATIVE, LABEL_FLAG_TOO_LARGE = \
    capi.LABEL_FLAG_NOT_INTEGRAL, capi.LABEL_FLAG_NEGATIVE, capi.LABEL_FLAG_TOO_LARGE


def label_bytes(hdr: NiftiHeader) -> int:
    """The width ``read_label_map`` decodes a file to: 1 byte for the 1-byte datatypes, else 2."""
    return 1 if hdr.bytes_per_voxel == 1 else 2


def labels_on_host(hdr: NiftiHeader, raw: np.ndarray, out_bytes: Optional[int] = None) -> Tuple[np.ndarray, int, int]:
    """numpy's statement of fnn_decode_labels -> (uint8 / uint16 (z, y, x), flags, largest valid label).  The value judged
    is ``decode_on_host``'s float32 (an integer datatype without scaling is judged as the integer); a voxel that is no label
    - not integral or not finite (1), else negative (2), else above the type's maximum (4) - is 0 and raises its flag."""
    out_bytes = label_bytes(hdr) if out_bytes is None else int(out_bytes)
    top = 255 if out_bytes == 1 else 65535
    if hdr.dtype_char[0] in 'iu' and not hdr.scale:
        v = np.frombuffer(memoryview(raw).cast('B')[:hdr.n_bytes], dtype=np.dtype(hdr.endian + hdr.dtype_char)).astype(np.int64)
        odd = np.zeros(v.shape, bool)
    else:
        v = decode_on_host(hdr, raw).reshape(-1)
        with np.errstate(invalid='ignore'):
            odd = ~np.isfinite(v) | (v != np.trunc(v))
    with np.errstate(invalid='ignore'):
        neg = ~odd & (v < 0)
        big = ~odd & (v > top)
    flags = (LABEL_FLAG_NOT_INTEGRAL if odd.any() else 0) | (LABEL_FLAG_NEGATIVE if neg.any() else 0) | \
        (LABEL_FLAG_TOO_LARGE if big.any() else 0)
    labels = np.where(odd | neg | big, 0, v).astype(np.uint8 if out_bytes == 1 else np.uint16)
    return labels.reshape(hdr.shape), flags, int(labels.max()) if labels.size else 0


def label_flags_error(fname: str, flags: int, out_bytes: int) -> RuntimeError:
    said = []
    if flags & LABEL_FLAG_NOT_INTEGRAL:
        said.append('voxels that are not integral or not finite')
    if flags & LABEL_FLAG_NEGATIVE:
        said.append('negative voxels')
    if flags & LABEL_FLAG_TOO_LARGE:
        said.append(f'voxels above {255 if out_bytes == 1 else 65535}, the largest label a {out_bytes}-byte map holds')
    return RuntimeError(f'{fname}: not a label file: it holds ' + ', '.join(said))


class ChunkedLayout:
    """Where the voxel stream of a ``.nii.gz`` file written with ``compress_on_device=True`` lies, for ``fnn_inflate_segments``:
    the raw deflate bytes ``file[first:first + in_bytes]`` inflate to the voxel bytes, ``starts`` (int64, relative to
    ``first``, ascending from 0) are the candidates for segment starts, ``header_crc`` is the CRC-32 of the ``vox_offset``
    bytes in front of the voxels and ``crc32`` the gzip trailer's, of all of them."""

    def __init__(self, first: int, in_bytes: int, starts: np.ndarray, header_crc: int, crc32: int):
        self.first, self.in_bytes, self.starts = int(first), int(in_bytes), starts
        self.header_crc, self.crc32 = int(header_crc), int(crc32)


CHUNK_MARKER = b'\x00\x00\xff\xff'                              # the empty stored block that ends a segment on a byte
HEADER_SEGMENT_SEARCH = 1 << 16                                  # the header's segment must end in the first 64 KiB of the file


def _marker_ends(blob: bytes, lo: int, hi: int) -> List[int]:
    found, at = [], blob.find(CHUNK_MARKER, lo, hi)
    while at >= 0:
        found.append(at + 4)
        at = blob.find(CHUNK_MARKER, at + 1, hi)
    return found


def _chunked_by_its_ends(head10: bytes, tail14: bytes) -> bool:
    """The O(1) test an ordinary zlib file fails: the gzip header ``write_label_file`` writes (magic, deflate, no flags), and a
    stream that ends with an empty stored block and the final empty fixed block in front of the trailer."""
    return len(head10) == 10 and head10[:4] == b'\x1f\x8b\x08\x00' and len(tail14) == 14 and tail14[:6] == CHUNK_MARKER + b'\x03\x00'


def chunked_layout(file_bytes, hdr: NiftiHeader) -> Optional[ChunkedLayout]:
    """The layout of a whole ``.nii.gz`` file for the device inflate, or None for a file that is not laid out as
    ``compressed_label_file_bytes`` lays it out (then the host inflates it, as ever).  Host only.  Nothing here is trusted
    later: the device call certifies the chain of segments and the sizes, the caller the CRC-32.

    * O(1) first: gzip magic, CM 8 and FLG 0 in the first 10 bytes, and ``file[-14:-8] == 00 00 FF FF 03 00``;
    * the trailer's ISIZE is ``(vox_offset + n_bytes) mod 2^32``;
    * the header's segment: the first end ``m`` of a marker 00 00 FF FF at which zlib inflates ``file[10:m]`` (closed with
      03 00) to exactly ``vox_offset`` bytes; markers are looked for in the first HEADER_SEGMENT_SEARCH bytes only;
    * the candidates: ``m`` and the end of every marker in ``file[m:len - 10]`` that lies below ``len - 10``."""
    blob = bytes(file_bytes)
    n = len(blob)
    if n < 10 + 5 + 6 + 8 or not _chunked_by_its_ends(blob[:10], blob[-14:]):
        return None
    crc, isize = struct.unpack('<II', blob[-8:])
    if isize != (hdr.vox_offset + hdr.n_bytes) & 0xFFFFFFFF:
        return None
    end = n - 10                                                 # the stream's end: behind the last marker, before 03 00
    for m in _marker_ends(blob, 10, min(end, 10 + HEADER_SEGMENT_SEARCH)):
        z = zlib.decompressobj(-15)
        try:
            head = z.decompress(blob[10:m] + b'\x03\x00', hdr.vox_offset + 1)
        except zlib.error:
            continue
        if z.eof and len(head) == hdr.vox_offset and not z.unused_data and not z.unconsumed_tail:
            break
    else:
        return None
    if m >= end:
        return None
    starts = np.array([m] + [e for e in _marker_ends(blob, m, end) if e < end], dtype=np.int64) - m
    return ChunkedLayout(m, end - m, starts, zlib.crc32(head), crc)


def gzip_member_start(blob: bytes) -> Optional[int]:
    """Where the deflate stream of a gzip member begins (RFC 1952): behind the 10 fixed bytes and what FLG announces - FEXTRA
    (a 2-byte length and that many bytes), FNAME and FCOMMENT (zero-terminated), FHCRC (2 bytes).  None for what is no gzip
    header of a deflate member, has a reserved flag set or ends inside its header."""
    n = len(blob)
    if n < 18 or blob[:3] != b'\x1f\x8b\x08' or blob[3] & 0xE0:
        return None
    flg, at = blob[3], 10
    if flg & 4:
        if at + 2 > n:
            return None
        at += 2 + struct.unpack_from('<H', blob, at)[0]
    for bit in (8, 16):
        if flg & bit:
            if at >= n:
                return None
            at = blob.find(b'\x00', at) + 1
            if at == 0:
                return None
    if flg & 2:
        at += 2
    return at if at < n - 8 else None


def stream_layout(file_bytes, hdr: NiftiHeader) -> Optional[ChunkedLayout]:
    """The layout of a whole ``.nii.gz`` file that anybody's zlib wrote, for ``fnn_inflate_stream``: the raw deflate bytes
    ``file[first:len - 8]`` are claimed to inflate to the ``vox_offset`` header bytes and the voxel bytes, ``crc32`` is the
    trailer's (``starts`` is None: the device finds where to begin).  None - the host inflates the file - for a header that
    ``gzip_member_start`` does not read, an ISIZE that is not ``(vox_offset + n_bytes) mod 2^32`` and a ``vox_offset`` that
    is no multiple of 16 (``fnn_decode_labels`` reads behind it).  A second member or bytes behind the trailer are not
    looked for here: the device call then ends with a status (the final block is not the input's end) and the host reads
    the file.  Nothing here is trusted later."""
    blob = bytes(file_bytes)
    first = gzip_member_start(blob)
    if first is None or hdr.vox_offset % 16:
        return None
    crc, isize = struct.unpack('<II', blob[-8:])
    if isize != (hdr.vox_offset + hdr.n_bytes) & 0xFFFFFFFF:
        return None
    return ChunkedLayout(first, len(blob) - 8 - first, None, 0, crc)


def inflate_on_device_value(value):
    """The ``inflate_on_device`` switch as the readers keep it: False, True, 'dynamic' or 'any'.  Any other string is a
    ValueError; what is no string counts by its truth, as before."""
    if isinstance(value, str):
        if value not in ('dynamic', 'any'):
            raise ValueError(f"inflate_on_device must be False, True, 'dynamic' or 'any', got {value!r}")
        return value
    return bool(value)


class StagedCase:
    """The files of one case between the host and the device: headers (checked), and one pinned byte buffer per file that a
    host thread fills.  ``layouts[i]`` is None when buffer i holds the file's voxel bytes, and the ``ChunkedLayout`` when it
    holds the whole compressed file for the device to inflate (label files of a reader with ``inflate_on_device``)."""

    def __init__(self, fnames, hdrs, buffers, inflate_on_device=False):
        self.fnames, self.hdrs, self.buffers = list(fnames), list(hdrs), list(buffers)
        self.inflate_on_device = bool(inflate_on_device)
        self.any_stream = inflate_on_device == 'any'             # files that are no chain of segments are staged too (stream_layout)
        self.layouts = [None] * len(self.fnames)

    def _stage_compressed(self, fname: str, hdr: NiftiHeader, buf) -> Optional[ChunkedLayout]:
        """The whole file into ``buf`` when it is a chunked ``.nii.gz`` that fits (the buffer is sized by the voxel bytes);
        with ``inflate_on_device='any'`` every other single-member ``.nii.gz`` that fits too (``stream_layout``)."""
        if not str(fname).lower().endswith('.nii.gz'):
            return None
        anybodys = self.any_stream
        with open(fname, 'rb') as f:
            size = os.fstat(f.fileno()).st_size
            if size > buf.numel() or size < 32:
                return None
            head10 = f.read(10)
            f.seek(size - 14)
            chunked = _chunked_by_its_ends(head10, f.read(14))
            if not chunked and not anybodys:
                return None
            f.seek(0)
            blob = f.read()
        layout = chunked_layout(blob, hdr) if chunked else None      # (the segment route: more parallelism)
        if layout is None and anybodys:
            layout = stream_layout(blob, hdr)
        if layout is not None:
            buf.numpy()[:len(blob)] = np.frombuffer(blob, dtype=np.uint8)
        return layout

    def fill(self):
        """Host only (file reads and zlib): may run on a thread."""
        for i, (f, h, b) in enumerate(zip(self.fnames, self.hdrs, self.buffers)):
            self.layouts[i] = self._stage_compressed(f, h, b) if self.inflate_on_device else None
            if self.layouts[i] is None:
                read_voxel_bytes(f, h, b.numpy())
        return self


class NiftiIO:
    """``read_images`` / ``read_seg`` / ``write_seg`` of the reference's reader-writer classes for single-file NIfTI-1."""
    supported_file_endings = list(SUPPORTED_FILE_ENDINGS)

    def __init__(self, device=None, inflate_on_device=False):
        self._device = device
        self._pinned = {}                            # slot -> list of pinned uint8 tensors, grown on demand
        # opt-in: label files written with compress_on_device=True are inflated by fnn_inflate_segments (csrc/inflate.hip)
        # instead of zlib; 'dynamic': by fnn_inflate_segments_dyn (csrc/inflate_dyn.hip), which also serves the files of
        # compress_on_device='dynamic'; 'any': those as with 'dynamic', and every other single-member .nii.gz - what zlib,
        # nibabel, SimpleITK or nnU-Net wrote - by fnn_inflate_stream (csrc/inflate_any.hip).  Which route each label file
        # took is counted here
        self.inflate_on_device = inflate_on_device_value(inflate_on_device)
        self.inflate_stats = {'device': 0, 'host': 0, 'fallback': 0}

    # ------------------------------------------------------------------ device side
    def _dev(self):
        import torch
        if self._device is None:
            if not torch.cuda.is_available():
                raise RuntimeError('NiftiIO decodes voxels on the GPU and none is visible '
                                   '(read_images(..., on_device=False) is the numpy route)')
            self._device = torch.device('cuda', torch.cuda.current_device())
        return torch.device(self._device)

    def stage(self, fnames: Sequence[str], slot: int = 0) -> StagedCase:
        """Headers read and checked, pinned staging buffers of slot ``slot`` sized for the case (allocated here, by the
        calling thread: the thread that later runs ``StagedCase.fill`` makes no GPU runtime call)."""
        hdrs = [read_header(f) for f in fnames]
        check_case(fnames, hdrs)
        return StagedCase(fnames, hdrs, self._pinned_buffers(hdrs, slot))

    def _pinned_buffers(self, hdrs: Sequence[NiftiHeader], slot: int):
        """One pinned byte buffer of slot ``slot`` per header, grown on demand."""
        import torch
        self._dev()
        bufs = self._pinned.setdefault(slot, [])
        for i, h in enumerate(hdrs):
            need = max(16, h.n_bytes)
            if i >= len(bufs):
                bufs.append(torch.empty(need, dtype=torch.uint8, pin_memory=True))
            elif bufs[i].numel() < need:
                bufs[i] = torch.empty(need, dtype=torch.uint8, pin_memory=True)
        return bufs[:len(hdrs)]

    def decode(self, staged: StagedCase):
        """A filled StagedCase -> (float32 ``[C, z, y, x]`` device tensor, properties).  Uploads every file's bytes and
        decodes them on the current stream, then synchronises: the staging buffers are free again on return."""
        import torch
        dev = self._dev()
        hdr0 = staged.hdrs[0]
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev)
            out = torch.empty((len(staged.hdrs), *hdr0.shape), dtype=torch.float32, device=dev)
            keep = []
            for c, (h, b) in enumerate(zip(staged.hdrs, staged.buffers)):
                raw = torch.empty(max(16, h.n_bytes), dtype=torch.uint8, device=dev)      # (the allocator aligns to 512 bytes)
                raw[:h.n_bytes].copy_(b[:h.n_bytes], non_blocking=True)
                capi.decode_voxels(raw.data_ptr(), h.datatype, h.byteswap, h.n_vox, h.scale, h.slope, h.inter,
                                   out[c].data_ptr(), stream.cuda_stream)
                keep.append(raw)
            stream.synchronize()
        return out, case_properties(hdr0)

    # ------------------------------------------------------------------ label files
    def stage_label_files(self, fnames: Sequence[str], slot: int = 0) -> StagedCase:
        """As ``stage`` for label files that are read one by one (a reference and a prediction, say): every header checked
        on its own, nothing compared between the files."""
        fnames = [str(f) for f in fnames]
        hdrs = [read_header(f) for f in fnames]
        staged = StagedCase(fnames, hdrs, self._pinned_buffers(hdrs, slot), self.inflate_on_device)
        self._orient_labels(staged)
        return staged

    def _orient_labels(self, staged: StagedCase) -> None:
        """What ``_label_frame`` needs to know about the files beyond their headers: here nothing."""

    def _label_frame(self, staged: StagedCase, i: int, labels):
        """File i's decoded map (device tensor or numpy array, in the file's frame) -> (the map as this class hands it out,
        its properties)."""
        return labels, case_properties(staged.hdrs[i])

    def decode_label_maps(self, staged: StagedCase) -> list:
        """A filled StagedCase -> per file ``(labels (z, y, x), properties)``: device tensors of uint8, or of int16 that carry
        the bits of uint16 (the engine's two-byte label type).  Every file's bytes are uploaded and decoded by
        ``fnn_decode_labels`` on the current stream - 1 byte wide for the 1-byte datatypes, else 2 bytes and narrowed to
        uint8 when the largest label is below 256.  RuntimeError naming the file when it holds what is no label.
        A file staged compressed (``inflate_on_device``) is uploaded as it is and inflated by ``fnn_inflate_segments``
        (``inflate_on_device='dynamic'``: ``fnn_inflate_segments_dyn``; ``'any'``: that, or ``fnn_inflate_stream`` for a file
        that is no chain of segments) into the same byte tensor; the result is taken only
        if the call certifies it (status 0) and its CRC-32, combined with the header's, is the gzip trailer's - anything else re-reads the file with zlib on this thread, which is the route the
        file takes without the flag and the one that says what is wrong with a corrupt file.
        Synchronises: the staging buffers are free again on return."""
        import torch
        dev = self._dev()
        n = len(staged.hdrs)
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev)
            status = torch.empty((max(n, 1), 2), dtype=torch.int32, device=dev)
            maps, keep = [], []
            for i, (h, b) in enumerate(zip(staged.hdrs, staged.buffers)):
                raw = torch.empty(max(16, h.n_bytes), dtype=torch.uint8, device=dev)      # (the allocator aligns to 512 bytes)
                if staged.layouts[i] is None:
                    self.inflate_stats['host'] += 1
                    inflated = None
                else:
                    inflated = self._inflate_staged(staged, i, raw, stream, keep)
                if inflated is None:
                    raw[:h.n_bytes].copy_(b[:h.n_bytes], non_blocking=True)
                    inflated = raw
                keep.append(raw)
                wide = label_bytes(h) == 2
                out = torch.empty(h.shape, dtype=torch.int16 if wide else torch.uint8, device=dev)
                capi.decode_labels(inflated.data_ptr(), h.datatype, h.byteswap, h.n_vox, h.scale, h.slope, h.inter, 2 if wide else 1,
                                   out.data_ptr(), status[i].data_ptr(), stream.cuda_stream)
                maps.append(out)
            said = status.cpu().numpy()                          # (waits for the stream)
            made = []
            for i, (f, h, m) in enumerate(zip(staged.fnames, staged.hdrs, maps)):
                if said[i, 0]:
                    raise label_flags_error(f, int(said[i, 0]), label_bytes(h))
                if m.dtype == torch.int16 and said[i, 1] < 256:
                    m = m.to(torch.uint8)
                made.append(self._label_frame(staged, i, m))
        return made

    def _inflate_staged(self, staged: StagedCase, i: int, raw, stream, keep: list):
        """File i, staged compressed -> the device tensor that holds its voxel bytes, made by the device inflate: ``raw`` for
        a chain of segments; for a stream that anybody's zlib wrote (``stream_layout``) the part behind ``vox_offset`` of a
        tensor of its own, which ``fnn_inflate_stream`` fills with the header bytes and the voxel bytes.  None: the device
        route refused it, and the staging buffer now holds the voxel bytes ``read_voxel_bytes`` made of the file."""
        import torch
        h, b, lay = staged.hdrs[i], staged.buffers[i], staged.layouts[i]
        comp = torch.empty(max(16, lay.in_bytes), dtype=torch.uint8, device=raw.device)
        comp[:lay.in_bytes].copy_(b[lay.first:lay.first + lay.in_bytes], non_blocking=True)
        keep.append(comp)
        if lay.starts is None:
            whole = torch.empty(h.vox_offset + max(16, h.n_bytes), dtype=torch.uint8, device=raw.device)
            keep.append(whole)
            status, crc = capi.inflate_stream(comp.data_ptr(), lay.in_bytes, whole.data_ptr(), h.vox_offset + h.n_bytes, stream.cuda_stream)
            certified, made = crc == lay.crc32, whole[h.vox_offset:]
        else:
            inflate = capi.inflate_segments if self.inflate_on_device is True else capi.inflate_segments_dyn
            status, crc = inflate(comp.data_ptr(), lay.in_bytes, lay.starts, raw.data_ptr(), h.n_bytes, stream.cuda_stream)
            certified, made = crc32_combine(lay.header_crc, crc, h.n_bytes) == lay.crc32, raw
        if status == capi.FNN_INFLATE_OK and certified:
            self.inflate_stats['device'] += 1
            return made
        self.inflate_stats['fallback'] += 1                      # (the call synchronised: the staging buffer is free)
        staged.layouts[i] = None
        read_voxel_bytes(staged.fnames[i], h, b.numpy())
        return None

    def read_label_map(self, fname: str, on_device: bool = True):
        """A label file as labels -> ``(labels (z, y, x), properties)``: on the device ``decode_label_maps``' tensor; with
        ``on_device=False`` the same values as a numpy uint8 / uint16 array, computed and checked with numpy (no GPU
        call).  A file with a voxel that is no label - not integral, negative, above the map's maximum - raises a
        RuntimeError that names it."""
        fname = str(fname)
        if on_device:
            return self.decode_label_maps(self.stage_label_files([fname]).fill())[0]
        hdr = read_header(fname)
        raw = np.empty(hdr.n_bytes, dtype=np.uint8)
        read_voxel_bytes(fname, hdr, raw)
        labels, flags, top = labels_on_host(hdr, raw)
        if flags:
            raise label_flags_error(fname, flags, label_bytes(hdr))
        if labels.dtype == np.uint16 and top < 256:
            labels = labels.astype(np.uint8)
        staged = StagedCase([fname], [hdr], [None])
        self._orient_labels(staged)
        return self._label_frame(staged, 0, labels)

    # ------------------------------------------------------------------ the reference's interface
    def read_images(self, image_fnames: Union[List[str], Tuple[str, ...]], on_device: bool = True):
        """-> (float32 ``[C, z, y, x]``, properties): a device tensor, or with ``on_device=False`` the same values as a
        numpy array computed on the host."""
        image_fnames = [str(f) for f in image_fnames]
        if on_device:
            return self.decode(self.stage(image_fnames).fill())
        hdrs = [read_header(f) for f in image_fnames]
        check_case(image_fnames, hdrs)
        images = []
        for f, h in zip(image_fnames, hdrs):
            raw = np.empty(h.n_bytes, dtype=np.uint8)
            read_voxel_bytes(f, h, raw)
            images.append(decode_on_host(h, raw)[None])
        return np.vstack(images), case_properties(hdrs[0])

    def read_seg(self, seg_fname: str, on_device: bool = True):
        return self.read_images((seg_fname,), on_device=on_device)

    def write_seg(self, seg, output_fname: str, properties: dict) -> None:
        write_nifti_seg(seg, output_fname, properties)

    def _file_frame_on_device(self, seg, properties: dict):
        """-> (the device label map in its file's frame, the affine its header takes)."""
        return seg, _affine_of(properties)

    def _compressible(self, seg, properties: dict, caller: str, host_route: str):
        """What both compress methods do first: the checks, then -> (the device label map in its file's frame, contiguous
        and 16-byte aligned; the affine its header takes)."""
        import torch
        if not hasattr(seg, 'data_ptr') or seg.device.type != 'cuda':
            raise TypeError(f'{caller} takes a label map on the GPU ({host_route} go to write_seg as they are)')
        assert seg.ndim == 3, 'segmentation must be 3d (z, y, x)'
        if seg.dtype not in (torch.uint8, torch.int16, torch.uint16):
            raise NotImplementedError(f'label maps of {seg.dtype} are not compressed on the device (uint8, int16 and uint16 are)')
        with torch.cuda.device(seg.device):
            seg, affine = self._file_frame_on_device(seg, properties)
            seg = seg.contiguous()
            return (seg.clone() if seg.data_ptr() % 16 else seg), affine

    def compress_labels(self, seg, properties: dict, tables: str = 'fixed') -> 'DeviceCompressedLabels':
        """A device label map (z, y, x; uint8, or the two-byte int16 / uint16) -> the deflate fragment of its voxels as the
        ``.nii.gz`` file holds them, made by ``fnn_deflate_labels`` on the current stream: what comes back from the device
        is the fragment, not the map.  The file type is ``_label_voxels``' (uint16 from a maximum of 255 on).  ``write_seg``
        takes the result.  Synchronises.
        ``tables='dynamic'``: ``fnn_deflate_labels_dyn`` - every chunk carries its own Huffman tables where they make it
        smaller.  Such a file is laid out in chunks as before (``chunked_layout`` recognises it); a reader with
        ``inflate_on_device='dynamic'`` inflates it on the device, while ``fnn_inflate_segments`` refuses dynamic blocks
        (``FNN_INFLATE_DYNAMIC``): a reader with ``inflate_on_device=True`` reads it with zlib, counted under
        ``inflate_stats['fallback']``.  Any other value of ``tables`` is a ValueError."""
        import torch
        if tables not in ('fixed', 'dynamic'):
            raise ValueError(f"tables must be 'fixed' or 'dynamic', got {tables!r}")
        deflate = capi.deflate_labels if tables == 'fixed' else capi.deflate_labels_dyn
        seg, affine = self._compressible(seg, properties, 'compress_labels', 'arrays on the host')
        with torch.cuda.device(seg.device):
            if seg.element_size() == 1 and seg.numel() > 0 and int(seg.max()) >= 255:
                seg = seg.to(torch.int16)                        # (a uint8 map that holds 255 is a uint16 file; a new, aligned tensor)
            n, size = seg.numel(), seg.element_size()
            cap = capi.deflate_bound(n * size)
            out = torch.empty(max(cap, 16), dtype=torch.uint8, device=seg.device)
            n_out, file_size, crc = deflate(seg.data_ptr(), size, n, True, out.data_ptr(), cap,
                                            torch.cuda.current_stream(seg.device).cuda_stream)[:3]
            fragment = out[:n_out].cpu().numpy().tobytes()
        return DeviceCompressedLabels(fragment, crc, n * file_size, tuple(seg.shape), file_size == 2, affine)

    def compress_label_masks(self, seg, labels: Sequence[int], properties: dict) -> List['DeviceCompressedLabels']:
        """A device label map (z, y, x; uint8, int16 or uint16) and label values -> per value the compressed uint8 mask
        ``seg == value`` as its ``.nii.gz`` file holds it, in the order of ``labels``: the map is brought to its file's frame
        once (``_file_frame_on_device``), ``fnn_deflate_masks_count`` sizes all fragments, ``fnn_deflate_masks_emit`` writes
        them into one buffer of exactly that size, and that buffer is what comes back from the device - neither the map nor
        a mask is downloaded.  ``write_seg`` takes each result.  Synchronises."""
        import torch
        labels = [int(i) for i in labels]
        seg, affine = self._compressible(seg, properties, 'compress_label_masks', 'masks of a host array')
        if not labels:
            return []
        with torch.cuda.device(seg.device):
            n, size, shape = seg.numel(), seg.element_size(), tuple(seg.shape)
            stream = torch.cuda.current_stream(seg.device).cuda_stream
            work_cap = capi.deflate_masks_work_bytes(n, len(labels))
            work = torch.empty(max(work_cap, 16), dtype=torch.uint8, device=seg.device)
            sizes, crcs = capi.deflate_masks_count(seg.data_ptr(), size, n, labels, work.data_ptr(), work_cap, stream)
            total = sum(sizes)
            out = torch.empty(max(total, 16), dtype=torch.uint8, device=seg.device)
            capi.deflate_masks_emit(seg.data_ptr(), size, n, labels, work.data_ptr(), out.data_ptr(), total, stream)
            blob = out[:total].cpu().numpy().tobytes()           # (the copy waits for the kernel on the stream)
        made, at = [], 0
        for nb, crc in zip(sizes, crcs):
            made.append(DeviceCompressedLabels(blob[at:at + nb], crc, n, shape, False, affine))
            at += nb
        return made


# ---------------------------------------------------------------------- writing
def _quaternion_of(affine: np.ndarray):
    """(qfac, zooms, (b, c, d)) of an affine's rotation part, as nibabel's ``set_qform`` derives them: column norms are the
    zooms, a left-handed matrix flips the third column (qfac = -1), the nearest orthogonal matrix (polar decomposition
    through the SVD) gives the unit quaternion - the eigenvector of the largest eigenvalue of Bar-Itzhack's symmetric
    matrix, with a >= 0."""
    rzs = np.asarray(affine, dtype=np.float64)[:3, :3]
    zooms = np.sqrt((rzs * rzs).sum(0))
    zooms = np.where(zooms == 0, 1.0, zooms)
    r = rzs / zooms
    qfac = 1.0
    if np.linalg.det(r) <= 0:
        qfac = -1.0
        r = r.copy()
        r[:, 2] *= -1
    p, _, q = np.linalg.svd(r)
    m = p @ q
    xx, yx, zx, xy, yy, zy, xz, yz, zz = m.reshape(-1)
    k = np.array([[xx - yy - zz, 0, 0, 0],
                  [yx + xy, yy - xx - zz, 0, 0],
                  [zx + xz, zy + yz, zz - xx - yy, 0],
                  [yz - zy, zx - xz, xy - yx, xx + yy + zz]]) / 3.0
    vals, vecs = np.linalg.eigh(k)
    x, y, z, w = vecs[:, np.argmax(vals)]
    if w < 0:
        x, y, z = -x, -y, -z
    return qfac, zooms, (x, y, z)


def nifti1_header_bytes(shape_xyz, datatype: int, affine: np.ndarray) -> bytes:
    """The 352 bytes (header + empty extension flag) of a little-endian single-file NIfTI-1 image of ``shape_xyz`` voxels with
    ``affine`` as the sform (code 2, 'aligned') and, with code 0, as the qform - what ``nibabel.Nifti1Image(array,
    affine)`` saves."""
    affine = np.asarray(affine, dtype=np.float64)
    qfac, zooms, quat = _quaternion_of(affine)
    h = bytearray(MIN_VOX_OFFSET)
    struct.pack_into('<i', h, 0, HEADER_BYTES)
    struct.pack_into('<8h', h, 40, 3, *[int(i) for i in shape_xyz], 1, 1, 1, 1)
    struct.pack_into('<2h', h, 70, int(datatype), 8 * DATATYPES[int(datatype)][1])
    struct.pack_into('<8f', h, 76, qfac, *[float(z) for z in zooms], 1.0, 1.0, 1.0, 1.0)
    struct.pack_into('<3f', h, 108, float(MIN_VOX_OFFSET), 1.0, 0.0)
    struct.pack_into('<2h', h, 252, 0, 2)
    struct.pack_into('<6f', h, 256, *[float(q) for q in quat], *[float(t) for t in affine[:3, 3]])
    struct.pack_into('<12f', h, 280, *[float(v) for v in affine[:3].reshape(-1)])
    h[344:348] = b'n+1\0'
    return bytes(h)


def _label_voxels(seg) -> Tuple[np.ndarray, bool]:
    """-> (contiguous uint8 array, or little-endian uint16 from a maximum of 255 on; is it uint16)."""
    seg = np.asarray(seg.cpu() if hasattr(seg, 'cpu') else seg)
    assert seg.ndim == 3, 'segmentation must be 3d (z, y, x)'
    u16 = seg.size > 0 and np.max(seg) >= 255
    return np.ascontiguousarray(seg.astype('<u2' if u16 else np.uint8, copy=False)), u16


# ---- labels compressed on the device
GZIP_HEADER = bytes.fromhex('1f8b08000000000004ff')              # what GzipFile(filename='', mtime=0, compresslevel=1) writes
_CRC_POLY = 0xEDB88320


def _crc_mulmod(a: int, b: int) -> int:
    """a * b modulo the CRC-32 polynomial, both in the reflected representation (bit 31 is x^0)."""
    p = 0
    for i in range(32):
        if a & (0x80000000 >> i):
            p ^= b
        b = (b >> 1) ^ (_CRC_POLY if b & 1 else 0)
    return p


def crc32_combine(crc_a: int, crc_b: int, len_b: int) -> int:
    """``zlib.crc32(A + B)`` from ``zlib.crc32(A)``, ``zlib.crc32(B)`` and ``len(B)`` (zlib's crc32_combine, which Python does
    not expose): ``crc(A) * x^(8 len(B)) + crc(B)`` in the CRC's field, the power by repeated squaring."""
    power, square, e = 0x80000000, 0x40000000, 8 * int(len_b)    # x^0, x^1
    while e:
        if e & 1:
            power = _crc_mulmod(power, square)
        square = _crc_mulmod(square, square)
        e >>= 1
    return _crc_mulmod(int(crc_a), power) ^ int(crc_b)


class DeviceCompressedLabels:
    """A label map in its file's frame that was compressed on the device: the deflate ``fragment`` of its voxel bytes
    (byte aligned, not final), their ``crc32`` and count ``n_bytes``, the map's ``shape`` (z, y, x), whether the file is
    ``uint16``, and the ``affine`` its header takes.  The writer only assembles the file around it."""

    def __init__(self, fragment: bytes, crc32: int, n_bytes: int, shape, uint16: bool, affine: np.ndarray):
        self.fragment, self.crc32, self.n_bytes = bytes(fragment), int(crc32), int(n_bytes)
        self.shape, self.uint16, self.affine = tuple(int(i) for i in shape), bool(uint16), affine
        self.ndim = len(self.shape)


def compressed_label_file_bytes(labels: DeviceCompressedLabels, affine: Optional[np.ndarray] = None) -> bytes:
    """The ``.nii.gz`` file of ``labels``: one gzip member - the header ``write_label_file`` has always written; the NIfTI
    header as raw deflate, flushed to a byte without ending the stream; the device's fragment; the final empty fixed block;
    the CRC-32 of header plus voxels and their length modulo 2^32.  ``gzip.decompress`` gives the bytes of the host route's
    file."""
    head = nifti1_header_bytes(labels.shape[::-1], 512 if labels.uint16 else 2, labels.affine if affine is None else affine)
    z = zlib.compressobj(1, zlib.DEFLATED, -15)
    head_z = z.compress(head) + z.flush(zlib.Z_SYNC_FLUSH)
    crc = crc32_combine(zlib.crc32(head), labels.crc32, labels.n_bytes)
    return b''.join((GZIP_HEADER, head_z, labels.fragment, b'\x03\x00',
                     struct.pack('<II', crc, (len(head) + labels.n_bytes) & 0xFFFFFFFF)))


def _affine_of(properties: dict) -> np.ndarray:
    if 'nibabel_stuff' in properties:
        return properties['nibabel_stuff']['original_affine']
    if 'sitk_stuff' in properties:
        return affine_from_sitk_stuff(properties['sitk_stuff'])
    raise RuntimeError('write_seg: the properties carry neither nibabel_stuff nor sitk_stuff')


def write_label_file(seg, output_fname: str, affine: np.ndarray) -> None:
    """``seg`` (z, y, x), in the file's own frame, as a NIfTI-1 label file with ``affine``; a ``DeviceCompressedLabels`` is
    only assembled and written (``.nii.gz`` names only).  The file appears under its name only when it is complete."""
    gz = _check_ending(output_fname)
    compressed = isinstance(seg, DeviceCompressedLabels)
    if compressed:
        if not gz:
            raise ValueError(f'{output_fname}: labels compressed on the device make a .nii.gz file')
        blob = compressed_label_file_bytes(seg, affine)
    else:
        data, u16 = _label_voxels(seg)
        head = nifti1_header_bytes(data.shape[::-1], 512 if u16 else 2, affine)
    tmp = f'{output_fname}.part{os.getpid()}'
    try:
        with open(tmp, 'wb') as f:
            if compressed:
                f.write(blob)
            elif gz:
                with gzip.GzipFile(filename='', mode='wb', compresslevel=1, fileobj=f, mtime=0) as g:
                    g.write(head)
                    g.write(memoryview(data).cast('B'))
            else:
                f.write(head)
                f.write(memoryview(data).cast('B'))
        os.replace(tmp, output_fname)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)


def write_nifti_seg(seg, output_fname: str, properties: dict) -> None:
    """``NibabelIO.write_seg``: ``seg`` (z, y, x) as uint8 (uint16 from a maximum of 255 on) with the case's affine
    (``nibabel_stuff`` if the properties have it, else rebuilt from ``sitk_stuff``).  The file appears under its name
    only when it is complete."""
    _check_ending(output_fname)
    if isinstance(seg, DeviceCompressedLabels):
        return write_label_file(seg, output_fname, seg.affine)
    write_label_file(seg, output_fname, _affine_of(properties))


# ---------------------------------------------------------------------- orientation (NibabelIOWithReorient)
# nibabel's orientation rules, restated from its published behaviour (orientations.py: io_orientation, ornt_transform,
# inv_ornt_aff, apply_orientation; SpatialImage.as_reoriented) - nibabel is not a dependency and none of this is pinned
# against it.  An orientation is a (3, 2) float array: row i = (the output axis the array's axis i lies along, +1 / -1),
# in nibabel's (x, y, z) index space.
RAS_ORNT = np.array([[0.0, 1.0], [1.0, 1.0], [2.0, 1.0]])        # axcodes2ornt('RAS'): the identity


def io_orientation(affine: np.ndarray) -> np.ndarray:
    """The orientation of the array axes of ``affine`` relative to RAS+: columns of the 3x3 part divided by their norms
    (a zero norm counts as 1), replaced by the nearest orthogonal matrix (``P @ Qs`` of the SVD, singular values below
    ``S.max() * 3 * eps`` dropped); then the array axes in order each take the world axis with the largest absolute entry
    of their column, the direction its sign, and that world axis is taken out for the axes that follow."""
    rzs = np.asarray(affine, dtype=np.float64)[:3, :3]
    zooms = np.sqrt(np.sum(rzs * rzs, axis=0))
    zooms[zooms == 0] = 1
    rs = rzs / zooms
    p, s, qs = np.linalg.svd(rs, full_matrices=False)
    keep = s > s.max() * 3 * np.finfo(s.dtype).eps
    r = np.dot(p[:, keep], qs[keep])
    ornt = np.full((3, 2), np.nan)
    for in_ax in range(3):
        col = r[:, in_ax]
        if not np.allclose(col, 0):
            out_ax = int(np.argmax(np.abs(col)))
            ornt[in_ax] = [out_ax, -1.0 if col[out_ax] < 0 else 1.0]
            r[out_ax, :] = 0
    if np.isnan(ornt).any():
        raise RuntimeError(f'the affine\n{np.asarray(affine)}\nhas an array axis without a direction: no orientation')
    return ornt


def ornt_transform(start_ornt: np.ndarray, end_ornt: np.ndarray) -> np.ndarray:
    """The orientation that takes an array in ``start_ornt`` to ``end_ornt``."""
    out = np.empty((3, 2))
    for end_in, (end_out, end_flip) in enumerate(end_ornt):
        for start_in, (start_out, start_flip) in enumerate(start_ornt):
            if end_out == start_out:
                out[start_in] = [end_in, 1.0 if start_flip == end_flip else -1.0]
                break
        else:
            raise ValueError(f'Unable to find out axis {end_out} in start_ornt')
    return out


def inv_ornt_aff(ornt: np.ndarray, shape_xyz) -> np.ndarray:
    """The 4x4 matrix from indices of the array after ``ornt`` to indices of the array before it (``shape_xyz``: before)."""
    shape = np.array(shape_xyz[:3], dtype=np.float64)
    undo_reorder = np.eye(4)[[int(i) for i in ornt[:, 0]] + [3], :]
    undo_flip = np.diag(list(ornt[:, 1]) + [1.0])
    center = -(shape - 1) / 2.0
    undo_flip[:3, 3] = ornt[:, 1] * center - center
    return np.dot(undo_flip, undo_reorder)


def apply_orientation(arr_xyz: np.ndarray, ornt: np.ndarray) -> np.ndarray:
    """numpy's route, in nibabel's index space: every axis whose direction is -1 flipped, then ``transpose(argsort(ornt[:, 0]))``."""
    out = np.asarray(arr_xyz)
    for ax in range(3):
        if ornt[ax, 1] == -1:
            out = np.flip(out, ax)
    return out.transpose(np.argsort(ornt[:, 0]))


def is_identity_ornt(ornt: np.ndarray) -> bool:
    return bool(np.array_equal(ornt, RAS_ORNT))


def reorient_args(ornt: np.ndarray) -> Tuple[Tuple[int, int, int], Tuple[int, int, int]]:
    """``(src_axis, flip)`` of ``fnn_reorient`` (and of ``reorient_on_host``) for the engine's arrays - the one place where
    nibabel's index space meets the engine's.  An engine array is (z, y, x): its axis d is nibabel's axis 2 - d.  The
    reoriented array's nibabel axis o is the original's axis ``inv[o]`` (``inv = argsort(ornt[:, 0])``), counted backwards
    when ``ornt[inv[o], 1]`` is -1; so output axis d = 2 - o reads input axis ``2 - inv[2 - d]``."""
    inv = np.argsort(ornt[:, 0])
    src = tuple(2 - int(inv[2 - d]) for d in range(3))
    flip = tuple(int(ornt[int(inv[2 - d]), 1] == -1) for d in range(3))
    return src, flip


def reorient_on_host(arr_zyx: np.ndarray, src_axis, flip) -> np.ndarray:
    """numpy's statement of fnn_reorient: ``out[i] = arr[j]``, ``j[src_axis[d]] = i[d]``, counted backwards where ``flip[d]``."""
    out = np.asarray(arr_zyx).transpose(src_axis)
    axes = tuple(d for d in range(3) if flip[d])
    return np.ascontiguousarray(np.flip(out, axes) if axes else out)


class Reorientation:
    """What ``as_reoriented(io_orientation(affine))`` does to one image of ``shape_xyz`` voxels, and the way back."""

    def __init__(self, affine: np.ndarray, shape_xyz, file_spacing: Optional[Sequence[float]] = None):
        self.original_affine = np.asarray(affine, dtype=np.float64)
        self.shape_xyz = tuple(int(i) for i in shape_xyz)
        self.ornt = io_orientation(self.original_affine)
        self.identity = is_identity_ornt(self.ornt)
        self.src_axis, self.flip = reorient_args(self.ornt)
        shape_zyx = self.shape_xyz[::-1]
        self.ras_shape = tuple(shape_zyx[a] for a in self.src_axis)          # (z, y, x) of the reoriented array
        if self.identity:
            # nibabel returns the image itself: its affine, and the zooms the file states
            self.reoriented_affine = self.original_affine.copy()
            self.spacing = None if file_spacing is None else [float(i) for i in file_spacing]
        else:
            self.reoriented_affine = np.dot(self.original_affine, inv_ornt_aff(self.ornt, self.shape_xyz))
            self.spacing = None
        if self.spacing is None:
            # the new image's header takes its zooms from the affine (set_qform): float32 column norms, reversed
            norms = np.sqrt(np.sum(self.reoriented_affine[:3, :3] ** 2, axis=0))
            self.spacing = [float(np.float32(i)) for i in norms[::-1]]


def restore_orientation(properties: dict, ras_shape_zyx) -> Tuple[Tuple[int, int, int], Tuple[int, int, int], np.ndarray]:
    """``NibabelIOWithReorient.write_seg``'s way back for a RAS-frame array of ``ras_shape_zyx``: ``(src_axis, flip)`` that
    bring it to the file's frame, and the restored affine ``reoriented_affine @ inv_ornt_aff(from_canonical, ras shape)``
    the written header carries (the reference saves that one, not ``original_affine``)."""
    stuff = properties['nibabel_stuff']
    from_canonical = ornt_transform(RAS_ORNT, io_orientation(stuff['original_affine']))
    src_axis, flip = reorient_args(from_canonical)
    reoriented = np.asarray(stuff['reoriented_affine'], dtype=np.float64)
    if is_identity_ornt(from_canonical):
        return src_axis, flip, reoriented
    restored = np.dot(reoriented, inv_ornt_aff(from_canonical, tuple(ras_shape_zyx)[::-1]))
    return src_axis, flip, restored


class FileFrameLabels:
    """A label map already in its file's frame, with the affine its header takes: what the calling thread of the file
    pipeline hands to the writer thread, which then only casts, compresses and writes."""

    def __init__(self, voxels_zyx: np.ndarray, affine: np.ndarray):
        self.voxels, self.affine = voxels_zyx, affine


def check_case_reoriented(fnames: Sequence[str], orients: Sequence[Reorientation]) -> None:
    """The files of one case after reorientation: equal shapes and spacings (RuntimeError), equal reoriented affines (a
    warning) - as the reference's NibabelIOWithReorient."""
    if any(o.ras_shape != orients[0].ras_shape for o in orients):
        raise RuntimeError(f'Not all input images have the same shape! Shapes: {[o.ras_shape for o in orients]} '
                           f'Image files: {list(fnames)}')
    if any(not np.array_equal(o.reoriented_affine, orients[0].reoriented_affine) for o in orients):
        warnings.warn(f'Not all input images have the same reoriented_affines! Affines: '
                      f'{[o.reoriented_affine for o in orients]} Image files: {list(fnames)}. It is up to you to decide '
                      f'whether that\'s a problem.')
    if any(o.spacing != orients[0].spacing for o in orients):
        raise RuntimeError(f'Not all input images have the same spacing_for_nnunet! This might be caused by them not '
                           f'having the same affine. spacings_for_nnunet: {[o.spacing for o in orients]} '
                           f'Image files: {list(fnames)}')


class NiftiReorientIO(NiftiIO):
    """The reference's ``NibabelIOWithReorient`` (imageio/nibabel_reader_writer.py:101-190): every image is brought to
    RAS+ on reading and the label map back to the file's frame on writing.  On the device both are one ``fnn_reorient``
    pass (csrc/reorient.hip) behind ``fnn_decode_voxels`` and before the download of the labels; an image that is RAS+
    already takes neither the pass nor the temporary."""

    @staticmethod
    def _orient(hdrs: Sequence[NiftiHeader]) -> List[Reorientation]:
        return [Reorientation(h.affine, h.shape_xyz, h.spacing) for h in hdrs]

    @staticmethod
    def _properties(o: Reorientation) -> dict:
        return {'nibabel_stuff': {'original_affine': o.original_affine.copy(), 'reoriented_affine': o.reoriented_affine.copy()},
                'spacing': list(o.spacing)}

    def stage(self, fnames: Sequence[str], slot: int = 0) -> StagedCase:
        """As ``NiftiIO.stage``; the case is checked after reorientation and carries its ``Reorientation`` per file."""
        hdrs = [read_header(f) for f in fnames]
        orients = self._orient(hdrs)
        check_case_reoriented(fnames, orients)
        staged = StagedCase(fnames, hdrs, self._pinned_buffers(hdrs, slot))
        staged.orients = orients
        return staged

    def decode(self, staged: StagedCase):
        """A filled StagedCase -> (float32 ``[C, *ras_shape]`` device tensor, properties): every file decoded into a
        temporary in the file's frame and reoriented into its channel (decoded straight into the channel when the file
        is RAS+ already).  Synchronises: the staging buffers are free again on return."""
        import torch
        dev = self._dev()
        o0 = staged.orients[0]
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev)
            out = torch.empty((len(staged.hdrs), *o0.ras_shape), dtype=torch.float32, device=dev)
            keep = []
            for c, (h, o, b) in enumerate(zip(staged.hdrs, staged.orients, staged.buffers)):
                raw = torch.empty(max(16, h.n_bytes), dtype=torch.uint8, device=dev)
                raw[:h.n_bytes].copy_(b[:h.n_bytes], non_blocking=True)
                keep.append(raw)
                if o.identity:
                    capi.decode_voxels(raw.data_ptr(), h.datatype, h.byteswap, h.n_vox, h.scale, h.slope, h.inter,
                                       out[c].data_ptr(), stream.cuda_stream)
                    continue
                tmp = torch.empty(h.shape, dtype=torch.float32, device=dev)
                keep.append(tmp)
                capi.decode_voxels(raw.data_ptr(), h.datatype, h.byteswap, h.n_vox, h.scale, h.slope, h.inter,
                                   tmp.data_ptr(), stream.cuda_stream)
                capi.reorient(tmp.data_ptr(), 4, h.shape, o.src_axis, o.flip, out[c].data_ptr(), stream.cuda_stream)
            stream.synchronize()
        return out, self._properties(o0)

    def _orient_labels(self, staged: StagedCase) -> None:
        staged.orients = self._orient(staged.hdrs)

    def _label_frame(self, staged: StagedCase, i: int, labels):
        """The map brought to RAS+: a device tensor by ``fnn_reorient`` on the current stream, a numpy array by numpy."""
        o = staged.orients[i]
        if hasattr(labels, 'data_ptr'):
            return self._reorient_on_device(labels, o.src_axis, o.flip), self._properties(o)
        return reorient_on_host(labels, o.src_axis, o.flip), self._properties(o)

    def read_images(self, image_fnames: Union[List[str], Tuple[str, ...]], on_device: bool = True):
        image_fnames = [str(f) for f in image_fnames]
        if on_device:
            return self.decode(self.stage(image_fnames).fill())
        hdrs = [read_header(f) for f in image_fnames]
        orients = self._orient(hdrs)
        check_case_reoriented(image_fnames, orients)
        images = []
        for f, h, o in zip(image_fnames, hdrs, orients):
            raw = np.empty(h.n_bytes, dtype=np.uint8)
            read_voxel_bytes(f, h, raw)
            images.append(reorient_on_host(decode_on_host(h, raw), o.src_axis, o.flip)[None])
        return np.vstack(images), self._properties(orients[0])

    @staticmethod
    def _restore(seg, properties: dict):
        """``restore_orientation`` for the RAS-frame map ``seg``; warns, as the reference, when the restored affine is not the file's."""
        src_axis, flip, restored = restore_orientation(properties, tuple(seg.shape))
        original = np.asarray(properties['nibabel_stuff']['original_affine'], dtype=np.float64)
        if not np.allclose(original, restored):
            warnings.warn(f'Restored affine does not match original affine.\nOriginal affine\n{original}\n'
                          f'Restored affine\n{restored}')
        return src_axis, flip, restored

    def labels_to_file_frame(self, seg, properties: dict) -> FileFrameLabels:
        """A RAS-frame label map (z, y, x) -> its file's frame with the restored affine.  A device tensor (uint8, or the
        two-byte int16 / uint16) is reoriented by ``fnn_reorient`` on the current stream and then downloaded; a numpy array
        is reoriented by numpy and no GPU call is made."""
        if hasattr(seg, 'data_ptr') and seg.device.type == 'cuda':
            seg, restored = self._file_frame_on_device(seg, properties)
            return FileFrameLabels(seg.cpu().numpy(), restored)
        src_axis, flip, restored = self._restore(seg, properties)
        return FileFrameLabels(reorient_on_host(seg.numpy() if hasattr(seg, 'data_ptr') else np.asarray(seg), src_axis, flip), restored)

    @staticmethod
    def _reorient_on_device(seg, src_axis, flip):
        """A device label map through ``fnn_reorient`` on the current stream (itself when there is nothing to do)."""
        import torch
        if src_axis == (0, 1, 2) and not any(flip):
            return seg
        if seg.element_size() not in (1, 2, 4):
            raise NotImplementedError(f'label maps of {seg.dtype} are not reoriented on the device (1-, 2- and 4-byte elements are)')
        with torch.cuda.device(seg.device):
            seg = seg.contiguous()
            out = torch.empty(tuple(seg.shape[a] for a in src_axis), dtype=seg.dtype, device=seg.device)
            capi.reorient(seg.data_ptr(), seg.element_size(), tuple(seg.shape), src_axis, flip, out.data_ptr(),
                          torch.cuda.current_stream(seg.device).cuda_stream)
            return out

    def _file_frame_on_device(self, seg, properties: dict):
        """The RAS-frame device label map brought to its file's frame by ``fnn_reorient``, and the restored affine: what
        ``compress_labels`` then compresses."""
        src_axis, flip, restored = self._restore(seg, properties)
        return self._reorient_on_device(seg, src_axis, flip), restored

    def write_seg(self, seg, output_fname: str, properties: dict) -> None:
        """``seg`` is in the RAS frame (z, y, x) like the reference's, or a ``FileFrameLabels`` made earlier by
        ``labels_to_file_frame``, or the ``DeviceCompressedLabels`` of ``compress_labels``.  The header carries the restored
        affine."""
        _check_ending(output_fname)
        if isinstance(seg, DeviceCompressedLabels):
            return write_label_file(seg, output_fname, seg.affine)
        if not isinstance(seg, FileFrameLabels):
            assert seg.ndim == 3, 'segmentation must be 3d (z, y, x)'
            seg = self.labels_to_file_frame(seg, properties)
        write_label_file(seg.voxels, output_fname, seg.affine)


# ---------------------------------------------------------------------- which class a plan or a file ending names
_NIFTI_CLASS_NAMES = ('NibabelIO', 'SimpleITKIO', 'NiftiIO')
_OTHER_CLASS_NAMES = ('NibabelIOWithReorient', 'SimpleITKIOWithReorient', 'NaturalImage2DIO', 'Tiff3DIO')


def reader_writer_class_by_name(name: str):
    """``recursive_find_reader_writer_by_name`` (imageio/reader_writer_registry.py:73-79) for this engine: the plain
    NIfTI readers of the reference are ``NiftiIO``; every other class is refused by name."""
    if name in _NIFTI_CLASS_NAMES:
        return NiftiIO
    if name in _OTHER_CLASS_NAMES:
        raise NotImplementedError(f'image reader-writer {name} is not implemented (NibabelIO and SimpleITKIO are, for '
                                  f'.nii and .nii.gz files; prediction_reader_writer_class also serves NibabelIOWithReorient)')
    raise NotImplementedError(f"Unable to find reader writer class '{name}': this engine implements NibabelIO and "
                              f"SimpleITKIO for .nii and .nii.gz files")


def determine_reader_writer_from_file_ending(file_ending: str):
    if str(file_ending).lower() in SUPPORTED_FILE_ENDINGS:
        return NiftiIO
    raise NotImplementedError(f'Unable to determine a reader for file ending {file_ending}: this engine reads '
                              f'.nii and .nii.gz')


def determine_reader_writer_from_dataset_json(dataset_json: dict):
    """imageio/reader_writer_registry.py:23-38 without the trial read of an example file."""
    name = dataset_json.get('overwrite_image_reader_writer')
    if name is not None and name != 'None':
        return reader_writer_class_by_name(name)
    return determine_reader_writer_from_file_ending(dataset_json['file_ending'])


def prediction_reader_writer_class(plans_manager, dataset_json: dict):
    """The reader-writer class ``nnUNetPredictor`` predicts from files with.  ``NibabelIOWithReorient`` - named by the plans'
    ``image_reader_writer`` or by the dataset's ``overwrite_image_reader_writer`` - is ``NiftiReorientIO``; everything else
    is what the registry functions above say: the plans' class, or for plans that name none the dataset's.
    (``SimpleITKIOWithReorient`` stays refused: it rests on ITK's DICOMOrient letters and on ITK's choice between qform and
    sform, neither of which can be checked here.)"""
    plans_name = plans_manager.plans.get('image_reader_writer')
    overwrite = dataset_json.get('overwrite_image_reader_writer')
    if 'SimpleITKIOWithReorient' in (plans_name, overwrite):
        return reader_writer_class_by_name('SimpleITKIOWithReorient')                 # (raises)
    if 'NibabelIOWithReorient' in (plans_name, overwrite):
        return NiftiReorientIO
    if plans_name is not None:
        return plans_manager.image_reader_writer_class
    return determine_reader_writer_from_dataset_json(dataset_json)
