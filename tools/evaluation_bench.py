"""Evaluation on one MI355X: the counting pass (fnn_confusion_counts) on a synthetic 512^3 61-label uint8 pair for 1 and
3 predictions, and determine_postprocessing per case over a handful of such cases, with the numpy restatement's seconds
on a smaller case next to them.

usage (repo root, GPU box): python tools/evaluation_bench.py [--n 512] [--cases 3] [--reps 10] [--out FILE]
Kernel times: run it under rocprofv3 --kernel-trace --stats.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from tools.postprocess_bench import make_map  # noqa: E402

COPY_RATE = 6.29e12            # B/s, MI355X_MICROARCH.md


def noisy(seg, seed, frac=0.002):
    rng = np.random.default_rng(seed)
    out = seg.copy()
    idx = rng.integers(0, out.size, int(out.size * frac))
    out.reshape(-1)[idx] = rng.integers(0, 61, idx.size).astype(np.uint8)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=512)
    ap.add_argument('--cases', type=int, default=3)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--cpu-n', type=int, default=192)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    from fast_nnunet_amd import capi
    from fast_nnunet_amd import evaluation as ev
    from fast_nnunet_amd import postprocessing as pp

    dev = torch.device('cuda', 0)
    values = list(range(1, 61))
    table = ev.class_table(values)
    ref = make_map(a.n)
    preds = [noisy(ref, 100 + k) for k in range(3)]
    d_ref = torch.from_numpy(ref).to(dev).reshape(-1)
    d_preds = [torch.from_numpy(p).to(dev).reshape(-1) for p in preds]
    stream = torch.cuda.current_stream(dev).cuda_stream
    lines = [f'evaluation_bench: {a.n}^3 uint8 maps, 61 labels (60 classes + other); '
             f'foreground voxels {int((ref > 0).sum())}; device {torch.cuda.get_device_name(dev)}',
             f'median of {a.reps} after one warm-up, CUDA events around the call (scratch allocation, count and copy-back '
             f'included)']
    for n_pred in (1, 3):
        ts = []
        for r in range(a.reps + 1):
            torch.cuda.synchronize(dev)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            capi.confusion_counts(d_ref.data_ptr(), [p.data_ptr() for p in d_preds[:n_pred]], False, d_ref.numel(),
                                  table, len(values), -1, stream)
            e1.record()
            torch.cuda.synchronize(dev)
            if r:
                ts.append(e0.elapsed_time(e1) * 1e3)
        us = float(np.median(ts))
        nbytes = d_ref.numel() * (1 + n_pred)
        lines.append(f'counting pass, {n_pred} prediction(s): {us:.1f} us, {nbytes / us / 1e6:.2f} TB/s effective '
                     f'({nbytes / 1e6:.0f} MB read; floor at the copy rate {nbytes / COPY_RATE * 1e6:.1f} us)')

    refs = [ref] + [make_map(a.n, seed=62 + k) for k in range(a.cases - 1)]
    cases_p = [noisy(r, 200 + k) for k, r in enumerate(refs)]
    dj = {'labels': {'background': 0, **{f'l{i}': i for i in range(1, 61)}}}
    pp.determine_postprocessing(cases_p[:1], refs[:1], dj)                       # warm-up
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    fns, kwargs = pp.determine_postprocessing(cases_p, refs, dj)
    torch.cuda.synchronize(dev)
    t = time.perf_counter() - t0
    lines.append(f'determine_postprocessing, {a.cases} cases of {a.n}^3 with 60 labels: {t / a.cases * 1e3:.0f} ms per '
                 f'case (host uploads included; 3 labellings + 1 counting pass of 4 predictions per case); '
                 f'{len(kwargs)} steps accepted')

    from evaluation_ref import HostBackend
    small = make_map(a.cpu_n, seed=70)
    sp = noisy(small, 300)
    t0 = time.perf_counter()
    pp.determine_postprocessing([sp], [small], dj, backend=HostBackend())
    t_host = time.perf_counter() - t0
    t0 = time.perf_counter()
    pp.determine_postprocessing([sp], [small], dj)
    torch.cuda.synchronize(dev)
    t_dev = time.perf_counter() - t0
    lines.append(f'{a.cpu_n}^3 case: numpy / scipy restatement (bincount counts, fused labelling, one thread) '
                 f'{t_host:.2f} s; device {t_dev * 1e3:.0f} ms')
    text = '\n'.join(lines)
    print(text)
    if a.out:
        with open(a.out, 'w') as fh:
            fh.write(text + '\n')


if __name__ == '__main__':
    main()
