"""A pure-Python restatement of the per-label mask encoder (csrc/deflate_masks.hip) on top of tests/deflate_ref.py.  Test
infrastructure only - nothing here is imported by the package.

The mask of label ``l`` is the uint8 array ``m[i] = (seg[i] == l)``.  Its fragment is a chain of independent chunks of CHUNK
mask bytes, as in deflate_ref, with one change:

* a chunk in which ``l`` occurs, and the last partial chunk always, is ``deflate_ref.chunk_bytes(mask_chunk, 1)``;
* a full chunk in which ``l`` does not occur is the constant ``ZERO_CHUNK``: block header, literal 0, 63 matches of length
  258 and one of 129 at distance 1, end-of-block, the empty stored block - 112 bytes where the segment rule takes 214.
"""
import numpy as np

import deflate_ref
from deflate_ref import CHUNK

ZERO_CHUNK_BYTES = 112


def zero_chunk() -> bytes:
    b = deflate_ref._Bits()
    b.put(0, 1)                                                   # BFINAL = 0
    b.put(1, 2)                                                   # BTYPE = 01
    b.symbol(0)
    for _ in range(63):
        b.match(258, 1)
    b.match(129, 1)
    b.symbol(256)                                                 # end of block
    b.put(0, 3)                                                   # BFINAL = 0, BTYPE = 00 ...
    b.to_byte()
    b.out += b'\x00\x00\xff\xff'                                  # ... of length 0
    return bytes(b.out)


ZERO_CHUNK = zero_chunk()


def work_bytes(n_elems: int, n_labels: int) -> int:
    """What ``fnn_deflate_masks_work_bytes`` returns (include/fnn.h states the formula)."""
    def r16(v):
        return (v + 15) // 16 * 16
    L, pairs = n_labels, n_labels * ((n_elems + CHUNK - 1) // CHUNK)
    return 384 + r16(4 * L) + r16(8 * (L + 1)) + r16(8 * L) + r16(4 * L) + 8 * pairs + r16(2 * pairs)


def mask_of(seg: np.ndarray, label: int) -> np.ndarray:
    return (np.asarray(seg).reshape(-1).astype(np.int64) == int(label)).astype(np.uint8)


def mask_fragment(seg: np.ndarray, label: int) -> bytes:
    """The device's fragment for the mask of ``label`` in the label map ``seg`` (any integer dtype, flattened in C order)."""
    mask = mask_of(seg, label)
    out = []
    for c in range(0, mask.size, CHUNK):
        piece = mask[c:c + CHUNK]
        if piece.size == CHUNK and not piece.any():
            out.append(ZERO_CHUNK)
        else:
            out.append(deflate_ref.chunk_bytes(piece.tobytes(), 1))
    return b''.join(out)


def present_pairs(seg: np.ndarray, labels) -> int:
    """The (chunk, label) pairs the device walks: the label occurs in the chunk, or the chunk is a last partial one."""
    flat = np.asarray(seg).reshape(-1)
    n = 0
    for c in range(0, flat.size, CHUNK):
        piece = flat[c:c + CHUNK]
        n += len(labels) if piece.size < CHUNK else int(np.isin(np.asarray(labels), piece).sum())
    return n
