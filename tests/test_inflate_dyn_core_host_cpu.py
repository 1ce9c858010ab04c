"""csrc/inflate_dyn_core.h says that its text compiles for the host: tests/inflate_dyn_core_host.cpp is that compilation, built
with the host's address and undefined-behaviour sanitizers where the compiler has them.  The segment rule that decodes
dynamic-Huffman blocks - the table header and its checks, the three canonical codes built serially in plain arrays, the
token loop it shares with csrc/inflate_core.h - runs there candidate after candidate and must give, record for record and
byte for byte, what the Python model (tests/inflate_dyn_ref.py) gives: on zlib's full-flush streams of the default strategy,
on the project's dynamic fragments, on hand-made table headers, with every byte position a candidate, and on truncated and
bit-flipped segments, where it must end cleanly with a reason every time.  A plain executable: nothing is loaded into
Python.  No GPU is involved."""
import os
import shutil
import struct
import subprocess
import zlib

import pytest

import inflate_dyn_cases as cases
import inflate_dyn_ref as ref

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope='module')
def host_decoder(tmp_path_factory):
    """The program, built once: with $CXX, else c++, else ROCm's clang++ (as tests/test_inflate_core_host_cpu.py), first with
    -fsanitize=address,undefined and, where the compiler or its runtime refuses that, without."""
    rocm = os.environ.get('ROCM_PATH', '/opt/rocm')
    found = [os.environ.get('CXX'), shutil.which('c++'), os.path.join(rocm, 'lib', 'llvm', 'bin', 'clang++'), os.path.join(rocm, 'llvm', 'bin', 'clang++')]
    cxx = next((c for c in found if c and (shutil.which(c) or os.path.isfile(c))), None)
    if cxx is None:
        pytest.fail('no C++ compiler: neither $CXX nor c++ nor ROCm\'s clang++')
    exe = str(tmp_path_factory.mktemp('inflate_dyn_core_host') / 'inflate_dyn_core_host')
    base = [cxx, '-std=c++17', '-O1', '-g', '-Wall', os.path.join(HERE, 'inflate_dyn_core_host.cpp'), '-o', exe]
    probe = struct.pack('<q', 0)
    for flags in (['-fsanitize=address,undefined', '-fno-sanitize-recover=all'], []):
        r = subprocess.run(base + flags, capture_output=True, text=True)
        if r.returncode == 0 and subprocess.run([exe], input=probe, capture_output=True).returncode == 0:
            break
    else:
        pytest.fail('inflate_dyn_core_host.cpp does not build: ' + r.stderr)

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


STREAMS = {**{k: v[0] for k, v in cases.zlib_streams().items()}, **{k: v[0] for k, v in cases.project_fragments().items()},
           **{k: v[0] for k, v in cases.fixed_only_streams().items()}}


@pytest.mark.parametrize('name', sorted(STREAMS))
def test_records_and_bytes_match_the_python_model(host_decoder, name):
    stream = STREAMS[name]
    starts = ref.candidates(stream)
    assert host_decoder(stream, starts) == model(stream, starts)


def test_hand_made_headers(host_decoder):
    for name, (stream, reason, made) in cases.hand_made().items():
        got = host_decoder(stream, [0])
        assert got == model(stream, [0]), name
        assert got[0][2] == reason and (made is None or got[0][1] == made), name


@pytest.mark.parametrize('name', ['zlib-texty-l9-k100', 'zlib-runs2-l6-k100', 'zlib-random-l1-k4096', 'labels1-32773', 'labels2-16385', 'fibonacci'])
def test_every_byte_position_as_a_candidate(host_decoder, name):
    stream = STREAMS[name][:3000]
    starts = list(range(len(stream)))
    assert host_decoder(stream, starts) == model(stream, starts)


def test_truncated_and_bit_flipped_segments_end_with_a_reason(host_decoder):
    """600 cases of the mutated corpus, candidates 0, six random positions and every marker's end: each ends with a reason
    (the program's exit code is 0, under the sanitizers where they were built in) and the records are the model's."""
    import numpy as np
    rng = np.random.default_rng(7)
    seen = set()
    for case, s in enumerate(cases.mutated(600)):
        starts = sorted(set([0] + [int(i) for i in rng.integers(0, len(s), 6)] + [e for e in ref.marker_ends(s) if e < len(s)]))
        got = host_decoder(s, starts)
        assert got == model(s, starts), case
        seen |= {r[2] for r in got}
    assert {ref.OK, ref.END, ref.TABLES, ref.SYMBOL, ref.DISTANCE} <= seen, seen
