"""csrc/deflate_core.h says that its text compiles for the host: tests/deflate_core_host.cpp is that compilation.  The lane
code both GPU encoders are made of - the token rule with its two readers, the counter, the bit writer, the CRC chain, the
zero chunk - runs there lane after lane and must give, byte for byte, the fragments of the Python models
(tests/deflate_ref.py, tests/deflate_masks_ref.py) and zlib's CRC-32.  No GPU is involved."""
import os
import shutil
import subprocess
import zlib

import numpy as np
import pytest

import deflate_masks_ref as masks_ref
import deflate_ref

HERE = os.path.dirname(os.path.abspath(__file__))
C, S = deflate_ref.CHUNK, deflate_ref.SEGMENT
LENGTHS = (0, 1, 2, 3, 255, 256, 257, 258, 259, C - 1, C, C + 1, 2 * C + 5)


@pytest.fixture(scope='module')
def host_encoder(tmp_path_factory):
    """The program, built once: with $CXX, else c++, else ROCm's clang++.  A machine without any of them could not have
    built the library either, so that is a failure and not a skip."""
    rocm = os.environ.get('ROCM_PATH', '/opt/rocm')
    found = [os.environ.get('CXX'), shutil.which('c++'), os.path.join(rocm, 'lib', 'llvm', 'bin', 'clang++'), os.path.join(rocm, 'llvm', 'bin', 'clang++')]
    cxx = next((c for c in found if c and (shutil.which(c) or os.path.isfile(c))), None)
    if cxx is None:
        pytest.fail('no C++ compiler: neither $CXX nor c++ nor ROCm\'s clang++')
    exe = str(tmp_path_factory.mktemp('deflate_core_host') / 'deflate_core_host')
    r = subprocess.run([cxx, '-std=c++17', '-O1', '-Wall', os.path.join(HERE, 'deflate_core_host.cpp'), '-o', exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

    def run(mode, data, label=None):
        out = subprocess.run([exe, mode] + ([] if label is None else [str(label)]), input=bytes(data), capture_output=True, check=True).stdout
        return int.from_bytes(out[:4], 'little'), out[4:]
    return run


def _no_runs(n):
    """Bytes below 144 of which none equals the one or the two before it."""
    return (np.arange(n) % 3 * 40 + np.arange(n) // 3 % 37).astype(np.uint8)


def _constant(n):
    return np.full(n, 7, np.uint8)


def _runs_of_1_2_3(n):
    reps = np.tile([1, 2, 3], n // 6 + 1)
    return np.repeat((np.arange(reps.size) * 11 % 120).astype(np.uint8), reps)[:n]


def _run_across_boundaries(n):
    """One value from 6 bytes before to 6 bytes behind the first segment boundary, and the same around the first chunk boundary."""
    d = _no_runs(n)
    d[S - 6:S + 6] = 99
    d[C - 6:C + 6] = 98
    return d


def _nine_bit_literals(n):
    d = (144 + np.arange(n) * 5 % 112).astype(np.uint8)
    d[n // 3:n // 3 + 40] = 200                                     # ... and a match among them
    return d


def _low_bytes_repeat_at_distance_2(n):
    """The bytes of 2-byte labels 0x0105, 0x0205, 0x0305, ...: equal low bytes two apart, the elements differ; then runs of
    whole elements (also of one above 255)."""
    e = (np.arange((n + 1) // 2) % 7 * 256 + 0x105).astype('<u2')
    e[e.size // 2:] = np.repeat(np.array([3, 300, 3, 4], '<u2'), e.size // 8 + 1)[:e.size - e.size // 2]
    return e.view(np.uint8)[:n]


PATTERNS = (_constant, _runs_of_1_2_3, _run_across_boundaries, _nine_bit_literals, _low_bytes_repeat_at_distance_2)


@pytest.mark.parametrize('elem', (1, 2))
@pytest.mark.parametrize('pattern', PATTERNS, ids=lambda f: f.__name__.strip('_'))
def test_label_map_fragments_and_crcs_match_the_python_model(host_encoder, pattern, elem):
    for n in LENGTHS:
        data = pattern(n).tobytes()
        crc, frag = host_encoder(f'bytes{elem}', data)
        assert frag == deflate_ref.fragment(data, elem), (n, elem)
        assert crc == zlib.crc32(data), (n, elem)
        assert deflate_ref.inflate(frag) == data


def _label_map(n, dtype):
    """Runs of the labels 0 .. 4 everywhere; in the second chunk label 6 in one segment only (and, 2-byte maps, 300 in another)."""
    m = (np.arange(n) // 37 % 5).astype(dtype)
    m[C + 3 * S + 10:C + 4 * S - 10] = 6
    if np.dtype(dtype).itemsize == 2:
        m[C + 9 * S - 5:C + 9 * S + 5] = 300                       # (across a segment boundary)
    return m


@pytest.mark.parametrize('dtype,label', [('u1', 2), ('u1', 6), ('u1', 9), ('u1', 300), ('<u2', 2), ('<u2', 6), ('<u2', 9), ('<u2', 300), ('<u2', 262)],
                         ids=lambda v: str(v).strip('<'))
def test_mask_fragments_and_crcs_match_the_python_model(host_encoder, dtype, label):
    """Label 2: present in every chunk.  6 (and 300 in a 2-byte map): in one segment of the second chunk, so the first full
    chunk is the zero chunk and the last partial chunk is walked with the label absent.  9: nowhere.  300 in a 1-byte map and
    262 (low byte 6) in a 2-byte map: never equal to an element."""
    for n in LENGTHS:
        m = _label_map(n, dtype)
        crc, frag = host_encoder(f'mask{m.itemsize}', m.tobytes(), label)
        assert frag == masks_ref.mask_fragment(m, label), (n, dtype, label)
        assert crc == zlib.crc32(masks_ref.mask_of(m, label).tobytes()), (n, dtype, label)
    if label in (6, 9) or (label == 300 and m.itemsize == 2):
        assert frag.startswith(masks_ref.ZERO_CHUNK), 'the longest map\'s first chunk does not hold the label'
