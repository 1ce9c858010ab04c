"""The host code of fnn_instance_overlaps (csrc/instance.hip) as a plain executable: tests/instance_host.cpp is built with
hipcc for gfx950 like the library, with the host's address and undefined-behaviour sanitizers where the compiler and its runtime
take them, and run where it sees no GPU - nothing is loaded into Python.  Its tables and shape are heap blocks of their exact
size, so the argument checks cannot read past them unnoticed; with the pointer refusal let through, the call ends at the refused
allocation of its scratch.  tests/test_instance_refusals_cpu.py pins the same messages through the library."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope='module')
def instance_host(tmp_path_factory):
    """The program, built once; its environment hides every GPU, so that a machine that has one refuses the same calls."""
    hipcc = os.environ.get('HIPCC') or os.path.join(os.environ.get('ROCM_PATH', '/opt/rocm'), 'bin', 'hipcc')
    if not os.path.isfile(hipcc):
        pytest.fail('no hipcc: neither $HIPCC nor $ROCM_PATH/bin/hipcc')
    exe = str(tmp_path_factory.mktemp('instance_host') / 'instance_host')
    base = [hipcc, '-x', 'hip', '--offload-arch=gfx950', '-std=c++17', '-O1', '-g', '-Wall', '-Wno-unused-function',
            os.path.join(HERE, 'instance_host.cpp'), '-o', exe]
    env = dict(os.environ, HIP_VISIBLE_DEVICES='-1', ROCR_VISIBLE_DEVICES='-1')
    for flags in (['-Xarch_host', '-fsanitize=address,undefined', '-Xarch_host', '-fno-sanitize-recover=all'], []):
        r = subprocess.run(base + flags, capture_output=True, text=True)
        # `probe`: the HIP runtime starts and ends under this build (no check is made)
        if r.returncode == 0 and subprocess.run([exe, 'probe'], capture_output=True, env=env).returncode == 0:
            break
    else:
        pytest.fail('instance_host.cpp does not build: ' + r.stderr[-3000:])
    return lambda: subprocess.run([exe], capture_output=True, text=True, env=env)


def test_the_entrys_host_code_refuses_cleanly_without_a_gpu(instance_host):
    p = instance_host()
    assert p.returncode == 0, (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
    assert 'FAILED' not in p.stdout and 'skipped' not in p.stdout, p.stdout
    done = [line for line in p.stdout.splitlines() if line.startswith('ok ')]
    for who in ('refusals:', 'empty:', 'size:', 'pointers:', 'scratch:'):
        assert any(line.startswith('ok ' + who) for line in done), (who, p.stdout)
    assert p.stdout.rstrip().endswith('checks passed')
