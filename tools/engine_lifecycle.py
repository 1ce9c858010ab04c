"""Does an engine give back what it took?  Three lifecycles of tests/test_gpu_engine_lifecycle.py (build a predictor, every
path that makes the engine create a resource, close), and after each close the device's free memory plus what torch's
allocator holds: python tools/engine_lifecycle.py   (FNN_KNOBS=1 FNN_LIB=<another build> for an A-B, as tools/ab_libs.sh).
The figure is device-wide: other processes on the card move it."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'tests', 'golden')):
    sys.path.insert(0, p)

import torch  # noqa: E402

import test_gpu_engine_lifecycle as lc  # noqa: E402

x = lc._inputs()
torch.cuda.init()
first, figures = None, []
for cycle in range(1, 4):
    got = lc.one_cycle(x)
    if first is None:
        first = got
    lc._same(got, first)
    del got
    torch.cuda.synchronize()
    figures.append(torch.cuda.mem_get_info()[0] + torch.cuda.memory_reserved())
    print(f'cycle {cycle}: free + reserved after close = {figures[-1]} bytes')
lib = os.environ.get('FNN_LIB', "the tree's")
print(f'library {lib}: drop between cycle 1 and cycle 3 = {figures[0] - figures[2]} bytes')
