"""csrc/owned.h and csrc/host_upload.h are host code: tests/owned_host.cpp is built with hipcc for gfx950 like the library, with
the host's address and undefined-behaviour sanitizers where the compiler and its runtime take them, and run as a plain executable
that sees no GPU - nothing is loaded into Python.  There every HIP creation call is refused, which is the half of the owners the
GPU tests never reach: an owner stays empty after a refused creation and its destructor does nothing, ``reserve`` reports size 0,
``IntTable::upload`` and ``HostUpload::begin`` return the error and can be called again, ``HostUpload::finish(false)`` on an
upload that never began is harmless, and a move leaves its source empty.  tests/test_gpu_engine_lifecycle.py is the other half."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, '..', 'fast-nnunet_amd', 'csrc')


@pytest.fixture(scope='module')
def owned_host(tmp_path_factory):
    """The program, built once; its environment hides every GPU, so that a machine that has one refuses the same calls."""
    hipcc = os.environ.get('HIPCC') or os.path.join(os.environ.get('ROCM_PATH', '/opt/rocm'), 'bin', 'hipcc')
    if not os.path.isfile(hipcc):
        pytest.fail('no hipcc: neither $HIPCC nor $ROCM_PATH/bin/hipcc')
    exe = str(tmp_path_factory.mktemp('owned_host') / 'owned_host')
    base = [hipcc, '-x', 'hip', '--offload-arch=gfx950', '-std=c++17', '-O1', '-g', '-Wall', '-Wno-unused-function',
            os.path.join(HERE, 'owned_host.cpp'), os.path.join(CSRC, 'knob.hip'), '-o', exe]
    env = dict(os.environ, HIP_VISIBLE_DEVICES='-1', ROCR_VISIBLE_DEVICES='-1')
    for flags in (['-Xarch_host', '-fsanitize=address,undefined', '-Xarch_host', '-fno-sanitize-recover=all'], []):
        r = subprocess.run(base + flags, capture_output=True, text=True)
        # `probe`: the HIP runtime starts and ends under this build (no check is made)
        if r.returncode == 0 and subprocess.run([exe, 'probe'], capture_output=True, env=env).returncode == 0:
            break
    else:
        pytest.fail('owned_host.cpp does not build: ' + r.stderr[-3000:])
    return lambda: subprocess.run([exe], capture_output=True, text=True, env=env)


def test_owners_stay_empty_after_a_refused_creation_and_moves_empty_their_source(owned_host):
    p = owned_host()
    assert p.returncode == 0, (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
    assert 'FAILED' not in p.stdout and 'skipped' not in p.stdout, p.stdout
    done = [line for line in p.stdout.splitlines() if line.startswith('ok ')]
    for who in ('DevBuf:', 'PinnedBuf:', 'DevBuf::alloc:', 'Stream:', 'Event:', 'IntTable::upload:', 'HostUpload:', 'HostUpload::stage_copy:'):
        assert any(line.startswith('ok ' + who) for line in done), (who, p.stdout)
    assert p.stdout.rstrip().endswith('checks passed')
