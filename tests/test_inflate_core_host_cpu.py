"""csrc/inflate_core.h says that its text compiles for the host: tests/inflate_core_host.cpp is that compilation, built with
the host's address and undefined-behaviour sanitizers where the compiler has them.  The decode step the GPU kernels are made
of - bit reader, fixed code, bases and extras, the segment rule and its reasons - runs there candidate after candidate and
must give, record for record and byte for byte, what the Python model (tests/inflate_ref.py) gives: on the project's own
fragments, on zlib's Z_FIXED full-flush streams, with every byte position a candidate, and on truncated and bit-flipped
streams, where it must end cleanly with a reason every time.  A plain executable: nothing is loaded into Python.  No GPU
is involved."""
import os
import shutil
import struct
import subprocess
import zlib

import numpy as np
import pytest

import deflate_masks_ref as masks_ref
import deflate_ref
import inflate_ref as ref

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope='module')
def host_decoder(tmp_path_factory):
    """The program, built once: with $CXX, else c++, else ROCm's clang++ (as tests/test_deflate_core_host_cpu.py), first with
    -fsanitize=address,undefined and, where the compiler or its runtime refuses that, without."""
    rocm = os.environ.get('ROCM_PATH', '/opt/rocm')
    found = [os.environ.get('CXX'), shutil.which('c++'), os.path.join(rocm, 'lib', 'llvm', 'bin', 'clang++'), os.path.join(rocm, 'llvm', 'bin', 'clang++')]
    cxx = next((c for c in found if c and (shutil.which(c) or os.path.isfile(c))), None)
    if cxx is None:
        pytest.fail('no C++ compiler: neither $CXX nor c++ nor ROCm\'s clang++')
    exe = str(tmp_path_factory.mktemp('inflate_core_host') / 'inflate_core_host')
    base = [cxx, '-std=c++17', '-O1', '-g', '-Wall', os.path.join(HERE, 'inflate_core_host.cpp'), '-o', exe]
    probe = struct.pack('<q', 0)
    for flags in (['-fsanitize=address,undefined', '-fno-sanitize-recover=all'], []):
        r = subprocess.run(base + flags, capture_output=True, text=True)
        if r.returncode == 0 and subprocess.run([exe], input=probe, capture_output=True).returncode == 0:
            break
    else:
        pytest.fail('inflate_core_host.cpp does not build: ' + r.stderr)

    def run(stream, starts):
        """-> per candidate ``(end, bytes made: the bytes themselves for a segment that was not refused, else their count, reason)``."""
        msg = struct.pack(f'<q{len(starts)}q', len(starts), *starts) + bytes(stream)
        p = subprocess.run([exe], input=msg, capture_output=True)
        assert p.returncode == 0, (p.returncode, p.stderr.decode()[-2000:])
        out, at, recs = p.stdout, 0, []
        for _ in starts:
            end, n, reason = struct.unpack_from('<qii', out, at)
            at += 16
            if reason == ref.OK:
                crc, = struct.unpack_from('<I', out, at)
                made = out[at + 4:at + 4 + n]
                assert crc == zlib.crc32(made), 'the CRC-32 folded from pieces of 260 bytes'
                at += 4 + n
                recs.append((end, made, reason))
            else:
                recs.append((end, n, reason))
        assert at == len(out)
        return recs
    return run


def model(stream, starts):
    made = []
    for s in starts:
        end, out, reason = ref.decode_segment(stream, s)
        made.append((end, out if reason == ref.OK else len(out), reason))
    return made


def _streams():
    """name -> (stream, the bytes it inflates to, or None for one that is no chain of segments)."""
    S = {}
    for elem in (1, 2):
        for n in (0, 1, 255, 16384, 16385, 2 * 16384 + 5):
            data = ref.label_runs(n, elem, seed=n)
            S[f'labels{elem}-{n}'] = (deflate_ref.fragment(data, elem), data)
    data = ref.random_bytes(16384 + 300, 3)
    S['nine-bit-literals'] = (deflate_ref.fragment(data, 1), data)
    m = (np.arange(3 * 16384 + 77) // 37 % 5).astype(np.uint8)
    m[16384 + 700:16384 + 900] = 6
    for label in (2, 6, 9):                                        # present everywhere; in one chunk (zero chunks around it); nowhere
        S[f'mask-{label}'] = (masks_ref.mask_fragment(m, label), masks_ref.mask_of(m, label).tobytes())
    for name, data in (('texty', ref.texty_bytes(40000, 1)), ('random', ref.random_bytes(20000, 2)), ('runs', ref.label_runs(40000, 2, 5))):
        for level in (1, 9):
            for k in (100, 4096, 16384):
                data_k = data[:3000] if k == 100 else data
                S[f'zlib-{name}-l{level}-k{k}'] = (ref.full_flush_stream(data_k, level, k), data_k)
    texty = ref.texty_bytes(40000, 1)
    S['dynamic'] = (ref.full_flush_stream(texty, 6, 4096, zlib.Z_DEFAULT_STRATEGY), None)
    S['sync-flush'] = (ref.full_flush_stream(texty, 6, 4096, flush=zlib.Z_SYNC_FLUSH), None)
    S['over-16k'] = (ref.full_flush_stream(texty, 1, 16385), None)
    S['truncated'] = (ref.full_flush_stream(texty, 1, 4096)[:-3], None)
    return S


STREAMS = _streams()


@pytest.mark.parametrize('name', sorted(STREAMS))
def test_records_and_bytes_match_the_python_model(host_decoder, name):
    stream, data = STREAMS[name]
    starts = ref.candidates(stream)
    got = host_decoder(stream, starts)
    assert got == model(stream, starts)
    if data is not None and stream:
        assert ref.chain(stream, starts, len(data))[:2] == (ref.OK, data)


@pytest.mark.parametrize('name', ['labels1-16385', 'labels2-255', 'mask-6', 'zlib-texty-l9-k100', 'zlib-random-l1-k100', 'dynamic'])
def test_every_byte_position_as_a_candidate(host_decoder, name):
    stream = STREAMS[name][0][:3000]
    starts = list(range(len(stream)))
    assert host_decoder(stream, starts) == model(stream, starts)


def test_truncated_and_bit_flipped_streams_end_with_a_reason(host_decoder):
    """A fixed seed, 300 cases, each a stream of a few hundred bytes cut short or with one to three bits flipped: every
    candidate ends with a reason (the program's exit code is 0, under the sanitizers where they were built in) and the
    records are the model's."""
    rng = np.random.default_rng(20240607)
    bases = [STREAMS[n][0] for n in ('labels1-255', 'labels2-16384', 'mask-2', 'zlib-texty-l9-k100', 'zlib-random-l1-k100', 'zlib-runs-l1-k100')]
    seen = set()
    for case in range(300):
        base = bases[case % len(bases)]
        at = int(rng.integers(0, max(1, len(base) - 400)))
        s = bytearray(base[at:at + int(rng.integers(8, 400))])
        if case % 3 == 0:
            s = s[:int(rng.integers(1, len(s) + 1))]
        else:
            for _ in range(int(rng.integers(1, 4))):
                s[int(rng.integers(0, len(s)))] ^= 1 << int(rng.integers(0, 8))
        starts = sorted(set([0] + [int(i) for i in rng.integers(0, len(s), 6)] + [e for e in ref.marker_ends(bytes(s)) if e < len(s)]))
        got = host_decoder(bytes(s), starts)
        assert got == model(bytes(s), starts), case
        seen |= {r[2] for r in got}
    assert {ref.OK, ref.END, ref.DISTANCE, ref.NLEN} <= seen, seen
