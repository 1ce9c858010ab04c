"""The torch resampling kernels (fnn_resample_torch, fnn_resample_torch_seg) on one MI355X: ms and effective GB/s -
bytes the pass has to move (input read once + output written once) over time - against the ~6.3 TB/s float4 copy rate
of MI355X HBM, for

* the export of the headline workload: 61 heads of fp16 logits from its network grid (spacing 2.0 x 0.977 x 0.977) to a
  512^3 cropped grid of a case scanned at 1.25 x 0.78 x 0.78 (network grid 320 x 410 x 410);
* a 2-channel fp32 image the other way (512^3 -> 320 x 410 x 410), and along a separate axis;
* a 118-label int16 segmentation the same way, under both rules;

and the default family (fnn_resample, order 1 and order 3; for the segmentation order 1 per label through
DevicePreprocessor.resample_seg) on the same shapes, for scale.

usage (repo root, GPU box): python tools/resample_torch_bench.py [--n 512] [--heads 61] [--reps 5] [--out FILE]
Kernel times: run it under rocprofv3 --kernel-trace --stats.
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_TBS = 6.29          # MI355X_MICROARCH: float4 copy, measured


def timed(fn, reps, dev):
    ts = []
    for r in range(reps + 1):                     # the first call is the warm-up
        torch.cuda.synchronize(dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        if r:
            ts.append(e0.elapsed_time(e1))
    return float(np.median(ts)), min(ts), max(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=512)
    ap.add_argument('--heads', type=int, default=61)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--labels', type=int, default=118)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    from fast_nnunet_amd import capi
    from fast_nnunet_amd.preprocess import DevicePreprocessor, compute_new_shape

    dev = torch.device('cuda', 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    pp = DevicePreprocessor(dev)
    n, H = a.n, a.heads
    raw_grid, raw_spacing, net_spacing = (n, n, n), (1.25, 0.78125, 0.78125), (2.0, 0.9765625, 0.9765625)
    net_grid = tuple(compute_new_shape(raw_grid, raw_spacing, net_spacing))
    lines = [f'resample_torch_bench: cropped grid {raw_grid}, network grid {net_grid}; device {torch.cuda.get_device_name(dev)}',
             f'median of {a.reps} after one warm-up, CUDA events on the stream; GB/s = (input bytes + output bytes) / time; '
             f'copy rate {COPY_TBS} TB/s']

    def report(name, ms, lo, hi, nbytes):
        gbs = nbytes / ms / 1e6
        lines.append(f'{name:<58s}: {ms:9.2f} ms  ({nbytes / 1e9:6.2f} GB, {gbs:7.0f} GB/s = '
                     f'{100 * gbs / (COPY_TBS * 1e3):5.1f} % of copy rate)  min {lo:.2f} max {hi:.2f}')
        print(lines[-1], flush=True)

    def image_runs(tag, x, new_shape, old_reps):
        out = torch.empty((x.shape[0], *new_shape), dtype=x.dtype, device=dev)
        nbytes = (x.numel() + out.numel()) * x.element_size()
        half = x.dtype == torch.half
        for axis in (None, 0):
            report(f'{tag}, fnn_resample_torch' + ('' if axis is None else f', separate axis {axis}'),
                   *timed(lambda: capi.resample_torch(x.data_ptr(), x.shape, new_shape, axis, half, out.data_ptr(), stream),
                          a.reps, dev), nbytes)
        for order in (1, 3):
            report(f'{tag}, fnn_resample order {order} (default family)',
                   *timed(lambda: capi.resample(x.data_ptr(), x.shape, new_shape, order, None, half, out.data_ptr(), stream),
                          old_reps, dev), nbytes)
        del out

    g = torch.Generator(device=dev).manual_seed(5)
    logits = torch.randn((H, *net_grid), generator=g, device=dev, dtype=torch.half) * 3
    image_runs(f'logits fp16 {H} x {net_grid} -> {raw_grid}', logits, raw_grid, 1)
    del logits
    torch.cuda.empty_cache()
    image = torch.randn((2, *raw_grid), generator=g, device=dev, dtype=torch.float32)
    image_runs(f'image fp32 2 x {raw_grid} -> {net_grid}', image, net_grid, 2)
    del image
    torch.cuda.empty_cache()

    # a blocky label map: coarse random labels enlarged by repetition (connected regions, every label present)
    coarse = torch.randint(0, a.labels, (1, n // 32, n // 32, n // 32), generator=g, device=dev, dtype=torch.int16)
    seg = coarse.repeat_interleave(32, 1).repeat_interleave(32, 2).repeat_interleave(32, 3).contiguous()
    out = torch.empty((1, *net_grid), dtype=torch.int16, device=dev)
    nbytes = (seg.numel() + out.numel()) * 2
    tag = f'segmentation int16 {a.labels} labels {raw_grid} -> {net_grid}'
    for memeff in (False, True):
        report(f'{tag}, fnn_resample_torch_seg' + (', memefficient' if memeff else ''),
               *timed(lambda: capi.resample_torch(seg.data_ptr(), seg.shape, net_grid, None, False, out.data_ptr(), stream,
                                                  is_seg=True, memefficient=memeff), a.reps, dev), nbytes)
    kw = {'is_seg': True, 'order': 1, 'order_z': 0, 'force_separate_z': None}
    report(f'{tag}, resample_seg order 1 (default family)',
           *timed(lambda: pp.resample_seg(seg, net_grid, raw_spacing, net_spacing, kw), 1, dev), nbytes)
    text = '\n'.join(lines)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
