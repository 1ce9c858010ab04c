"""Which kernel every conv layer gets, without a GPU: fnn_plan_table runs the engine's planning (the one place a conv
layer's kernel is chosen) for the sweep's plans (tools/plans/*.json) and the BASELINE workloads at their bench batch.
tests/golden/conv_choice.json holds the kernels one profiled forward per plan launched on an MI355X (fnn_kernel_log);
it matches the `picked` column of profiles/r06_plan_sweep.json."""
import glob
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from fast_nnunet_amd import capi  # noqa: E402
from fast_nnunet_amd.arch import spec_from_state_dict  # noqa: E402

GOLDEN = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'conv_choice.json')))
PLANS = {os.path.basename(p)[:-5]: p for p in sorted(glob.glob(os.path.join(ROOT, 'tools', 'plans', '*.json')))}
WORKLOADS = {'bone_turbo_r2': ('bone_turbo_r2', 'f16'), 'iso128_r2': ('iso128_r2', 'f16'), 'iso128_teacher': ('iso128_teacher', 'f16'),
             'resenc160_r2': ('resenc160_r2', 'f16'), 'resenc160_r2_f8': ('resenc160_r2', 'f8')}


class _Args:
    def __init__(self, plan, workload):
        self.plan, self.workload, self.volume, self.batch, self.batch_given = plan, workload, 512, 32, False


def plan_desc(name):
    """-> (bench batch, fnn_arch_desc) of a sweep plan or BASELINE workload; tests/test_layer_plan_cpu.py plans the same"""
    plan, (workload, dtype) = PLANS.get(name), WORKLOADS.get(name, (None, 'f16'))
    args = _Args(plan, workload)
    w = bench.resolve_workload(args)
    strides, kernels = bench.plan_topology(w['spacing'], w['patch'])
    n = len(strides)
    features = [max(min(w['max_features'], 32 * 2 ** i) // w['r'], 8) for i in range(n)]
    if w['resenc']:
        blocks = (list(bench.RESENC_BLOCKS) + [bench.RESENC_BLOCKS[-1]] * n)[:n]
        sd = bench.synthetic_resenc_checkpoint(features, kernels, strides, blocks, w['in_channels'], w['heads'], seed=1234)
    else:
        sd = bench.synthetic_checkpoint(features, kernels, strides, w['in_channels'], w['heads'], seed=1234)
    spec = spec_from_state_dict(sd, w['patch'])
    spec.precision = capi.FNN_PREC_F8 if dtype == 'f8' else capi.FNN_PREC_F16
    return args.batch, spec.to_desc()


def _plan_rows(name):
    batch, desc = plan_desc(name)
    return batch, capi.plan_table(desc, batch)


@pytest.mark.parametrize('name', sorted(GOLDEN))
def test_each_conv_layer_gets_the_kernel_it_launched(name):
    batch, rows = _plan_rows(name)
    assert batch == GOLDEN[name]['batch']
    picked = {str(r['index']): r['picked'] for r in rows if r['type'] == 'conv'}
    assert picked == GOLDEN[name]['conv']
    assert all(r['picked'] == '-' for r in rows if r['type'] != 'conv')
    # the CPU twin of test_gpu_plans.py's last assert: no plan reaches the generic kernel
    assert not any('generic' in k for k in picked.values()), picked


def test_every_plan_and_workload_is_pinned():
    assert set(GOLDEN) == set(PLANS) | set(WORKLOADS)
