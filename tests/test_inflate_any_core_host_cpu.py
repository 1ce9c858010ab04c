"""csrc/inflate_any_core.h says that its text compiles for the host: tests/inflate_any_core_host.cpp is that compilation, built
with the host's address and undefined-behaviour sanitizers where the compiler has them.  The block finder, the member rule,
the chain, the 16-bit entries with their markers (through a ring of 32768 slots, as the emit kernel keeps one), the windows
and the resolved bytes run there pass by pass and must give, record for record, what the Python model
(tests/inflate_any_ref.py) gives: on the stream matrix, on the hand-made streams and on truncated and bit-flipped streams,
where it must end with a reason every time.  A plain executable: nothing is loaded into Python.  No GPU is involved."""
import os
import shutil
import struct
import subprocess
import zlib

import pytest

import inflate_any_cases as cases
import inflate_any_ref as ref

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope='module')
def host_inflate(tmp_path_factory):
    """The program, built once as tests/test_inflate_dyn_core_host_cpu.py builds its own: with $CXX, else c++, else ROCm's
    clang++, first with -fsanitize=address,undefined and, where the compiler or its runtime refuses that, without."""
    rocm = os.environ.get('ROCM_PATH', '/opt/rocm')
    found = [os.environ.get('CXX'), shutil.which('c++'), os.path.join(rocm, 'lib', 'llvm', 'bin', 'clang++'), os.path.join(rocm, 'llvm', 'bin', 'clang++')]
    cxx = next((c for c in found if c and (shutil.which(c) or os.path.isfile(c))), None)
    if cxx is None:
        pytest.fail('no C++ compiler: neither $CXX nor c++ nor ROCm\'s clang++')
    exe = str(tmp_path_factory.mktemp('inflate_any_core_host') / 'inflate_any_core_host')
    base = [cxx, '-std=c++17', '-O1', '-g', '-Wall', os.path.join(HERE, 'inflate_any_core_host.cpp'), '-o', exe]
    probe = struct.pack('<q', 0)
    for flags in (['-fsanitize=address,undefined', '-fno-sanitize-recover=all'], []):
        r = subprocess.run(base + flags, capture_output=True, text=True)
        if r.returncode == 0 and subprocess.run([exe], input=probe, capture_output=True).returncode == 0:
            break
    else:
        pytest.fail('inflate_any_core_host.cpp does not build: ' + r.stderr)

    def run(stream, out_bytes):
        """-> (candidates, records, status, members or None, windows, bytes, crc)."""
        p = subprocess.run([exe], input=struct.pack('<q', out_bytes) + bytes(stream), capture_output=True)
        assert p.returncode == 0, (p.returncode, p.stderr.decode()[-2000:])
        out, at = p.stdout, 0

        def take(fmt):
            nonlocal at
            v = struct.unpack_from(fmt, out, at)
            at += struct.calcsize(fmt)
            return v
        n, = take('<q')
        cand = list(take(f'<{n}q'))
        recs = [take('<qqii') for _ in range(n)]
        status, = take('<i')
        if status != ref.OK:
            assert at == len(out)
            return cand, recs, status, None, None, None, None
        k, = take('<q')
        members = []
        for _ in range(k):
            start, off, ln = take('<qqq')
            members.append((start, off, list(take(f'<{ln}H'))))
        windows = []
        for _ in range(max(k - 1, 0)):
            windows.append(out[at:at + ref.WINDOW])
            at += ref.WINDOW
        made = out[at:at + out_bytes]
        at += out_bytes
        crc, = take('<I')
        assert at == len(out)
        return cand, recs, status, members, windows, made, crc
    return run


def agree(host_inflate, stream, out_bytes):
    """The program's passes against the model's, record for record -> the status."""
    cand, recs, status, members, windows, made, crc = host_inflate(stream, out_bytes)
    r = ref.inflate(stream, out_bytes)
    assert cand == r.candidates
    known = set(cand)
    for p, rec in zip(cand, recs):
        end, entries, reason, reach = ref.decode_member(stream, p, out_bytes, known)
        assert rec == (end, len(entries), reason, reach), p
    assert status == r.status, (ref.REASONS[status], ref.REASONS[r.status])
    if status == ref.OK:
        assert members == [(m[0], m[1], m[3]) for m in r.members]
        assert windows == r.windows
        assert made == r.data and crc == r.crc
    return status


@pytest.mark.parametrize('kind', cases.KINDS + ('own',))
def test_records_entries_windows_and_bytes_match_the_python_model(host_inflate, kind):
    for name, (stream, data) in cases.matrix().items():
        if name.split('-')[0] == kind:
            assert agree(host_inflate, stream, len(data)) == ref.OK, name
            assert zlib.crc32(data) == host_inflate(stream, len(data))[6], name


def test_hand_made_streams(host_inflate):
    for name, (stream, out_bytes, status, _) in cases.hand_made().items():
        assert agree(host_inflate, stream, out_bytes) == status, name


def test_a_wrong_out_bytes_is_size_or_output(host_inflate):
    for name in ('runs1-32769-l6-m1', 'ct-65541-l6-m1', 'random-255-l0', 'runs2-65541-l6-fixed', 'own-dynamic2-32769'):
        stream, data = cases.matrix()[name]
        for wrong in (len(data) - 1, len(data) + 1):
            assert agree(host_inflate, stream, wrong) in (ref.SIZE, ref.OUTPUT), name


def test_truncated_and_bit_flipped_streams_end_with_a_reason(host_inflate):
    """400 cases of the mutated corpus: each ends with a reason (the program's exit code is 0, under the sanitizers where they
    were built in) and every record is the model's."""
    seen = set()
    for stream, out_bytes in cases.mutated(400):
        seen.add(agree(host_inflate, stream, out_bytes))
    assert {ref.OK, ref.END, ref.TABLES, ref.SYMBOL, ref.DISTANCE, ref.FINAL, ref.SIZE, ref.OUTPUT} <= seen, seen
