"""The word rule of fnn_binary_morphology (csrc/morph_core.h) as a plain executable: tests/morph_core_host.cpp is built with the
host C++ compiler under the address and undefined-behaviour sanitizers (without them where the compiler or its runtime does
not take them) and run - nothing is loaded into Python.  It compares every bit of the packed planes with a byte-wise brute
force for all four operations, the three ranks, both border values and n = 1..3 on rows with and without a tail, and on boxes
that touch 0, 1 or 2 faces of the volume per axis."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope='module')
def morph_core_host(tmp_path_factory):
    cxx = os.environ.get('CXX') or shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    if not cxx:
        rocm_clang = os.path.join(os.environ.get('ROCM_PATH', '/opt/rocm'), 'llvm', 'bin', 'clang++')
        cxx = rocm_clang if os.path.isfile(rocm_clang) else None
    if not cxx:
        pytest.fail('no host C++ compiler: neither $CXX, c++, g++, clang++ nor ROCm\'s clang++')
    exe = str(tmp_path_factory.mktemp('morph_core_host') / 'morph_core_host')
    base = [cxx, '-std=c++17', '-O1', '-g', '-Wall', os.path.join(HERE, 'morph_core_host.cpp'), '-o', exe]
    for flags in (['-fsanitize=address,undefined', '-fno-sanitize-recover=all'], []):
        r = subprocess.run(base + flags, capture_output=True, text=True)
        if r.returncode == 0:
            break
    else:
        pytest.fail('morph_core_host.cpp does not build: ' + r.stderr[-3000:])
    return lambda: subprocess.run([exe], capture_output=True, text=True)


def test_the_word_rule_of_binary_morphology(morph_core_host):
    p = morph_core_host()
    assert p.returncode == 0, (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
    assert 'FAILED' not in p.stdout, p.stdout
    done = [line for line in p.stdout.splitlines() if line.startswith('ok ')]
    for who in ('words:', 'tails:', 'boxes:'):
        assert any(line.startswith('ok ' + who) for line in done), (who, p.stdout)
    assert p.stdout.rstrip().endswith('checks passed')
