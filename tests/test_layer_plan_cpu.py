"""The layer plan (csrc/layer_plan.hip) without a GPU, through fnn_plan_table: every column of every row for the sweep's
plans and the BASELINE workloads at default switches, the same for the plan switches on the plans they change, and every
refusal of planning by exception type and message.  tests/golden/layer_plan_rows.json was recorded from the library of the
commit before the plan became a value of its own (`FNN_KNOBS=1 FNN_LIB=<that library> python tests/test_layer_plan_cpu.py`),
so the rows pin what that library planned.

The rows are made in one child process started with FNN_KNOBS=1 and no other FNN_* switch: the library latches only
FNN_KNOBS and reads every other switch when it plans, so the child changes its environment between plans.  It never opens
a GPU."""
import ctypes as C
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fast_nnunet_amd import capi  # noqa: E402

GOLDEN = __name__ != '__main__' and json.load(open(os.path.join(ROOT, 'tests', 'golden', 'layer_plan_rows.json')))   # (the child makes rows only)
DEFAULT = sorted(json.load(open(os.path.join(ROOT, 'tests', 'golden', 'conv_choice.json'))))
VARIANTS = [('FNN_NO_FUSE=1', ['iso128_r2', 'aniso_96x160x160_r2']),
            ('FNN_FUSE_STEM=0', ['iso128_r2', 'aniso_96x160x160_r2']),
            ('FNN_FUSE_STEM=1', ['iso128_r2', 'aniso_96x160x160_r2']),
            ('FNN_STEM_DIRECT=1', ['brats_128_c4_r1', 'plane2d_512_r2']),
            ('FNN_NO_POOL_FUSE=1', ['resenc128_r1']),
            ('FNN_CONV_V1=1', ['hippocampus_40x56x40_r1']),
            ('FNN_NO_ROW=1', ['prostate_20x320x256_r2']),
            ('FNN_FP8_LEVELS=12', ['resenc160_r2_f8'])]
KEYS = DEFAULT + [f'{name} {switch}' for switch, names in VARIANTS for name in names]


def _table(desc, batch):
    """fnn_plan_table's rows as text: [[12 columns] per layer]"""
    lib = capi.load_library()
    n = capi.check(lib.fnn_plan_table(C.byref(desc), int(batch), None, 0), lib)
    buf = C.create_string_buffer(int(n))
    lib.fnn_plan_table(C.byref(desc), int(batch), buf, n)
    return [r.split('\t') for r in buf.value.decode().split('\n') if r]


def _all_rows():
    """(in the child process) {key: rows} for KEYS"""
    from test_conv_choice_cpu import plan_desc
    descs = {}

    def rows(name):
        if name not in descs:
            descs[name] = plan_desc(name)
        batch, desc = descs[name]
        return _table(desc, batch)

    out = {name: rows(name) for name in DEFAULT}
    for switch, names in VARIANTS:
        var, value = switch.split('=')
        os.environ[var] = value
        for name in names:
            out[f'{name} {switch}'] = rows(name)
        del os.environ[var]
    return out


@pytest.fixture(scope='module')
def planned():
    env = {k: v for k, v in os.environ.items() if not k.startswith('FNN_') or k == 'FNN_LIB'}
    env['FNN_KNOBS'] = '1'
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout)


def test_the_fixture_holds_every_plan_and_variant():
    assert sorted(GOLDEN) == sorted(KEYS) and len(DEFAULT) == 21
    assert all(len(row) == 12 for rows in GOLDEN.values() for row in rows)


@pytest.mark.parametrize('key', KEYS)
def test_the_plan_has_the_recorded_rows(planned, key):
    assert planned[key] == GOLDEN[key]


def _toy(**fields):
    """A small valid PlainConvUNet descriptor; fields: scalars, or {stage: value} for the per-stage arrays"""
    d = capi.ArchDesc()
    d.kind, d.n_stages, d.in_channels, d.num_heads = capi.FNN_NET_PLAIN, 3, 1, 3
    strides = [(1, 1, 1), (2, 2, 2), (1, 2, 2)]
    for s in range(3):
        d.features[s], d.n_conv_enc[s], d.n_conv_dec[s] = (8, 16, 16)[s], 2, 2
        for a in range(3):
            d.kernels[s][a], d.strides[s][a] = 3, strides[s][a]
    d.patch[0], d.patch[1], d.patch[2] = 16, 16, 32
    d.eps, d.slope, d.spatial_dims, d.precision = 1e-5, 0.01, 3, capi.FNN_PREC_F16
    for name, value in fields.items():
        if isinstance(value, dict):
            for s, v in value.items():
                if isinstance(v, tuple):
                    for a in range(3):
                        getattr(d, name)[s][a] = v[a]
                else:
                    getattr(d, name)[s] = v
        elif isinstance(value, tuple):
            for a in range(3):
                getattr(d, name)[a] = value[a]
        else:
            setattr(d, name, value)
    return d


_2D = dict(spatial_dims=2, patch=(1, 16, 32), kernels={s: (1, 3, 3) for s in range(3)}, strides={1: (1, 2, 2)})
REFUSALS = [
    ('unknown kind', dict(kind=7), NotImplementedError, 'unknown network kind 7'),
    ('one stage', dict(n_stages=1), AssertionError, 'n_stages out of range'),
    ('too many stages', dict(n_stages=capi.FNN_MAX_STAGES + 1), AssertionError, 'n_stages out of range'),
    ('no input channel', dict(in_channels=0), NotImplementedError, 'in_channels must be 1..4096'),
    ('4097 input channels', dict(in_channels=4097), NotImplementedError, 'in_channels must be 1..4096'),
    ('no head', dict(num_heads=0), NotImplementedError, 'num_heads must be 1..256'),
    ('257 heads', dict(num_heads=257), NotImplementedError, 'num_heads must be 1..256'),
    ('kernel of 5', dict(kernels={1: (3, 5, 3)}), NotImplementedError, 'kernel sizes must be 1 or 3'),
    ('stride of 3', dict(strides={1: (2, 3, 2)}), NotImplementedError, 'strides must be 1 or 2'),
    ('strided stage 0', dict(strides={0: (1, 2, 2)}), NotImplementedError, 'stage 0 must have stride 1'),
    ('one spatial dim', dict(spatial_dims=1), AssertionError, 'spatial_dims must be 2 or 3'),
    ('2-D with a deep patch', dict(_2D, patch=(2, 16, 32)), AssertionError, 'a 2-D configuration has patch[0] == 1'),
    ('2-D with a depth kernel', dict(_2D, kernels={0: (1, 3, 3), 1: (3, 3, 3), 2: (1, 3, 3)}), AssertionError,
     'a 2-D configuration has kernel and stride 1 along the first axis'),
    ('patch not divisible', dict(patch=(16, 16, 34)), AssertionError, 'patch size 34 is not divisible by the pooling of axis 2'),
    ('no conv in an encoder stage', dict(n_conv_enc={1: 0}), AssertionError, 'n_conv_per_stage must be >= 1'),
    ('no block in a residual stage', dict(kind=capi.FNN_NET_RESENC, n_conv_enc={1: 0}), AssertionError, 'n_blocks_per_stage must be >= 1'),
    ('no conv in a decoder stage', dict(n_conv_dec={1: 0}), AssertionError, 'n_conv_per_stage_decoder must be >= 1'),
    ('batch of 0', dict(), AssertionError, 'max_batch must be 1..512 for this patch size'),
]


def test_the_descriptors_the_refusals_start_from_are_planned():
    assert len(_table(_toy(), 2)) == 12                     # 6 encoder convs, 2 x (transposed conv + 2 convs)
    assert len(_table(_toy(**_2D), 2)) == 13                # + the patches' windows as a tensor in front of the stem
    assert len(_table(_toy(kind=capi.FNN_NET_RESENC), 2)) > 12


@pytest.mark.parametrize('what, fields, exc, message', REFUSALS, ids=[r[0] for r in REFUSALS])
def test_planning_refuses(what, fields, exc, message):
    with pytest.raises(exc) as info:
        _table(_toy(**fields), 0 if what == 'batch of 0' else 2)
    assert type(info.value) is exc and str(info.value) == message


if __name__ == '__main__':
    print(json.dumps(_all_rows(), sort_keys=True).replace('], ', '],\n'))              # one table row per line
