"""csrc/deflate_dyn_core.h says that its text compiles for the host: tests/deflate_dyn_host.cpp is that compilation.  The
code the kernels of csrc/deflate_dyn.hip are made of - the histogram walk, df_code_lengths, the table header, the choice, the
canonical codes, the emitter - runs there lane after lane and must give, byte for byte, the fragments of the Python model
(tests/deflate_dyn_ref.py) and zlib's CRC-32.  A second mode feeds frequency vectors straight to df_code_lengths at the
limits 15 and 7.  The program is built twice, the second time with -fsanitize=address,undefined (the arrays of the serial
merge are where an overrun would hide), and both run the same inputs; it has its own main and nothing is preloaded.
No GPU is involved.

The 7-bit limit of the code-length code is reached twice: by the frequency vectors, and by a chunk that a random search
found (deflate_dyn_ref.deep_header_chunk), which the GPU test runs too."""
import os
import shutil
import subprocess
import zlib

import numpy as np
import pytest

import deflate_dyn_ref as dyn
import deflate_ref
from test_deflate_core_host_cpu import LENGTHS, PATTERNS

HERE = os.path.dirname(os.path.abspath(__file__))
C, S = deflate_ref.CHUNK, deflate_ref.SEGMENT


@pytest.fixture(scope='module', params=('plain', 'sanitized'))
def host_encoder(request, tmp_path_factory):
    """The program, built once per kind: with $CXX, else c++, else ROCm's clang++ (the compiler search of
    test_deflate_core_host_cpu.py)."""
    rocm = os.environ.get('ROCM_PATH', '/opt/rocm')
    found = [os.environ.get('CXX'), shutil.which('c++'), os.path.join(rocm, 'lib', 'llvm', 'bin', 'clang++'), os.path.join(rocm, 'llvm', 'bin', 'clang++')]
    cxx = next((c for c in found if c and (shutil.which(c) or os.path.isfile(c))), None)
    if cxx is None:
        pytest.fail('no C++ compiler: neither $CXX nor c++ nor ROCm\'s clang++')
    exe = str(tmp_path_factory.mktemp('deflate_dyn_host') / f'deflate_dyn_host_{request.param}')
    flags = ['-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-g'] if request.param == 'sanitized' else []
    r = subprocess.run([cxx, '-std=c++17', '-O1', '-Wall', *flags, os.path.join(HERE, 'deflate_dyn_host.cpp'), '-o', exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

    def run(mode, data, *args):
        r = subprocess.run([exe, mode, *[str(a) for a in args]], input=bytes(data), capture_output=True)
        assert r.returncode == 0, r.stderr.decode(errors='replace')[-2000:]
        return r.stdout
    return run


def _fragment(host_encoder, data, elem):
    out = host_encoder(f'bytes{elem}', data)
    return int.from_bytes(out[:4], 'little'), int.from_bytes(out[4:8], 'little'), out[8:]


def _few_labels(n):
    """What a label map is made of: a handful of values in runs of 40 to 300."""
    rng = np.random.default_rng(5)
    k = n // 40 + 2
    return np.repeat(rng.integers(0, 6, k), rng.integers(40, 300, k))[:n].astype(np.uint8)


def _random(n):
    return np.random.default_rng(6).integers(0, 256, n, dtype=np.uint8)


@pytest.mark.parametrize('elem', (1, 2))
@pytest.mark.parametrize('pattern', PATTERNS + (_few_labels, _random), ids=lambda f: f.__name__.strip('_'))
def test_fragments_and_crcs_match_the_python_model(host_encoder, pattern, elem):
    dynamic = 0
    for n in LENGTHS:
        data = pattern(n).tobytes()
        crc, dynamic_chunks, frag = _fragment(host_encoder, data, elem)
        want, want_dynamic = dyn.fragment(data, elem)
        assert dynamic_chunks == want_dynamic, (n, elem)
        assert frag == want, (n, elem)
        assert crc == zlib.crc32(data), (n, elem)
        assert deflate_ref.inflate(frag) == data
        dynamic += dynamic_chunks
    assert dynamic > 0, 'some chunk of every pattern takes its own tables'


def test_the_fibonacci_chunk_and_the_tiny_chunk(host_encoder):
    for data, want_dynamic in ((dyn.fibonacci_chunk(), 1), (dyn.TINY_CHUNK, 0)):
        crc, dynamic_chunks, frag = _fragment(host_encoder, data, 1)
        assert (frag, dynamic_chunks) == dyn.fragment(data, 1) and dynamic_chunks == want_dynamic
        assert crc == zlib.crc32(data) and deflate_ref.inflate(frag) == data


def _fibonacci(n):
    f = [1, 1]
    while len(f) < n:
        f.append(f[-1] + f[-2])
    return f[:n]


def _vectors(n):
    rng = np.random.default_rng(n)
    heavy = [1] * n
    heavy[n // 2] = 30000
    sparse = [0] * n
    sparse[1], sparse[n - 2] = 7, 3
    return {'fibonacci': _fibonacci(min(n, 40)) + [0] * (n - min(n, 40)), 'fibonacci_reversed': ([0] * (n - min(n, 40)) + _fibonacci(min(n, 40)))[::-1],
            'all_equal': [5] * n, 'two_symbols': sparse, 'one_heavy_symbol': heavy, 'one_symbol': [0] * (n - 1) + [9], 'none': [0] * n,
            'random': [int(v) for v in rng.integers(0, 2000, n)], 'powers': [2 ** min(i, 20) for i in range(n)]}    # (the sums stay below 2^31)


@pytest.mark.parametrize('n,limit', ((286, 15), (19, 7), (19, 15), (30, 7)))
def test_code_lengths_match_the_model_at_both_limits(host_encoder, n, limit):
    reached = False
    for name, freq in _vectors(n).items():
        got = list(host_encoder('lengths', np.array(freq, '<u4').tobytes(), limit))
        assert got == dyn.code_lengths(freq, limit), (name, n, limit)
        used = [g for g, f in zip(got, freq) if f]
        assert all(g == 0 for g, f in zip(got, freq) if not f) and all(1 <= g <= limit for g in used)
        if len(used) >= 2:
            assert sum(2 ** (limit - g) for g in used) == 2 ** limit, (name, 'Kraft with equality')
        reached |= max(got, default=0) == limit
    assert reached, 'some vector needs the limit'
    assert max(dyn.code_lengths(_vectors(n)['fibonacci'], limit)) == limit, 'Fibonacci frequencies are cut at the limit'


def test_a_chunk_whose_header_code_needs_the_seven_bit_limit(host_encoder):
    """A random search over skewed literal frequencies finds such chunks readily (this rule's trees take the merged node on
    a tie and so are deep).  tests/test_gpu_deflate_dyn.py runs the same chunk."""
    chunk = dyn.deep_header_chunk()
    clfreq = dyn.header_code_frequencies(chunk, 1)
    assert max(dyn.code_lengths(clfreq, 15)) > 7, 'without the limit the code-length code is too deep for its 3-bit fields'
    assert max(dyn.code_lengths(clfreq, 7)) == 7
    crc, dynamic_chunks, frag = _fragment(host_encoder, chunk, 1)
    assert (frag, dynamic_chunks) == dyn.fragment(chunk, 1) and dynamic_chunks == 1
    assert crc == zlib.crc32(chunk) and deflate_ref.inflate(frag) == chunk
