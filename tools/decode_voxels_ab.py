"""A-B of fnn_decode_voxels between two builds of the library in one process, on one MI355X: this tree's libfnn_hip.so and
another build given with --other (e.g. the same objects linked with the imageio.hip of an earlier commit: compile that file
to an object of its own and link it in place of imageio.o into a library of another name).  The two are called in turn, so
that clock and neighbours are shared: per datatype width, with and without scaling, with `out` on and one float past a
16-byte boundary; ms per call from `--calls` calls inside one pair of events, median (min, max) of `--windows` windows after
a warm-up window.  Both libraries are driven through ctypes alone: the other build need not export what capi.py binds.

usage (repo root, GPU box): python tools/decode_voxels_ab.py --other PATH/libfnn_other.so [--n 512] [--out FILE]
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--other', required=True)
    ap.add_argument('--other-name', default='other')
    ap.add_argument('--n', type=int, default=512)
    ap.add_argument('--calls', type=int, default=50)
    ap.add_argument('--windows', type=int, default=7)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r21_decode_voxels_ab.txt'))
    a = ap.parse_args()
    libs = {a.other_name: C.CDLL(os.path.abspath(a.other)), 'this': C.CDLL(os.path.join(ROOT, 'fast-nnunet_amd', 'csrc', 'libfnn_hip.so'))}
    for lib in libs.values():
        lib.fnn_decode_voxels.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int64, C.c_int, C.c_double, C.c_double, C.c_void_p, C.c_void_p]
    dev = torch.device('cuda', 0)
    n = a.n ** 3
    out = torch.empty(n + 4, dtype=torch.float32, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    lines = [f'decode_voxels_ab: fnn_decode_voxels on {a.n}^3 voxels, {" against ".join(libs)}, in turn in one process; device '
             f'{torch.cuda.get_device_name(dev)}',
             f'ms per call from {a.calls} calls inside one pair of events; median (min, max) of {a.windows} windows after a warm-up window; '
             f'scaling is slope 0.5, intercept -3']
    print('\n'.join(lines), flush=True)
    for code, size in ((2, 1), (4, 2), (8, 4), (16, 4), (64, 8)):
        raw = torch.randint(0, 200, (n * size,), dtype=torch.uint8, device=dev)
        for scale, off in ((0, 0), (0, 1), (1, 0)):
            ts = {k: [] for k in libs}
            for w in range(a.windows + 1):
                for k, lib in libs.items():
                    torch.cuda.synchronize(dev)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(a.calls):
                        if lib.fnn_decode_voxels(raw.data_ptr(), code, 0, n, scale, 0.5, -3.0, out.data_ptr() + 4 * off, stream) != 0:
                            sys.exit(f'fnn_decode_voxels failed in {k}')
                    e1.record()
                    e1.synchronize()
                    if w:
                        ts[k].append(e0.elapsed_time(e1) / a.calls)
            med = {k: float(np.median(v)) for k, v in ts.items()}
            lines.append(f'datatype {code:3d} scale {scale} out offset {off}: ' + '  '.join(
                f'{k} {med[k]:.4f} ms (min {min(v):.4f} max {max(v):.4f})' for k, v in ts.items()) +
                f'  this / {a.other_name} = {med["this"] / med[a.other_name]:.3f}')
            print(lines[-1], flush=True)
        del raw
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
