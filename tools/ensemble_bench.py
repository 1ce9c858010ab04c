"""Cross-configuration ensembling on one MI355X: ms and effective GB/s of fnn_ensemble_export for 61 heads on a 512^3
raw grid (crop = grid, fp16 logits), 2 and 5 members, labels only and with the averaged probabilities, against the
~6.3 TB/s float4 copy rate of MI355X HBM; and the numpy route (average_probabilities + argmax on host float32
probabilities) for comparison, on a smaller grid because one 61 x 512^3 float32 member alone is 32.7 GB.

usage (repo root, GPU box): python tools/ensemble_bench.py [--n 512] [--heads 61] [--members 2 5] [--reps 5]
                            [--numpy-n 128] [--out FILE] [--section export|resample]
Kernel times: run it under rocprofv3 --kernel-trace --stats.

--section resample: the step from the members' network-grid logits to the ensemble's labels, both ways in one process -
today's route (fnn_resample at order 1 per member into a fresh tensor of the cropped grid, then fnn_ensemble_export) and
the one fnn_ensemble_resample_export call - for fp16 members on the network grids 320 x 410 x 410 and 256^3 in turn,
default family, to a 512^3 crop = grid; with torch.cuda.max_memory_allocated of each route.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_TBS = 6.29          # MI355X_MICROARCH: float4 copy, measured


NETWORK_GRIDS = ((320, 410, 410), (256, 256, 256))


def _median_ms(fn, reps, dev):
    """Median, min and max of `reps` windows of fn() after one warm-up, events on the current stream."""
    ts = []
    for r in range(reps + 1):
        torch.cuda.synchronize(dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        if r:
            ts.append(e0.elapsed_time(e1))
    return float(np.median(ts)), min(ts), max(ts)


def resample_section(a, capi, dev):
    stream = torch.cuda.current_stream(dev).cuda_stream
    n, H = a.n, a.heads
    bbox, before, tb = [[0, n]] * 3, (n, n, n), (0, 1, 2)
    lines = [f'ensemble_bench --section resample: {H} heads, fp16 members on the network grids '
             f'{" / ".join("x".join(map(str, g)) for g in NETWORK_GRIDS)} in turn, default family (order 1, order_z 0), to a '
             f'{n}^3 crop = raw grid',
             f'device {torch.cuda.get_device_name(dev)}; median of {a.reps} windows after one warm-up, events on the stream around '
             f'the whole step; peak = torch.cuda.max_memory_allocated over one step (members\' network-grid logits, labels and '
             f'the average included)']
    g = torch.Generator(device=dev).manual_seed(5)
    logits = []
    labels = torch.empty((n, n, n), dtype=torch.uint8, device=dev)
    rows = [(N, False) for N in sorted(a.members)] + [(min(a.members), True)]
    for N, with_avg in rows:
        while len(logits) < N:
            logits.append(torch.randn((H, *NETWORK_GRIDS[len(logits) % 2]), generator=g, device=dev, dtype=torch.half) * 3)
        members = logits[:N]
        avg = torch.empty((H, n, n, n), dtype=torch.float32, device=dev) if with_avg else None
        avg_ptr = None if avg is None else avg.data_ptr()

        def two_step():
            resampled = []
            for lg in members:
                out = torch.empty((H, n, n, n), dtype=torch.half, device=dev)
                capi.resample(lg.data_ptr(), lg.shape, (n, n, n), 1, None, True, out.data_ptr(), stream, order_z=0)
                resampled.append(out)
            capi.ensemble_export([t.data_ptr() for t in resampled], [True] * N, H, None, bbox, before, tb, avg_ptr,
                                 labels.data_ptr(), False, stream)

        def fused():
            capi.ensemble_resample_export([(lg.data_ptr(), True, lg.shape[1:], capi.FNN_RESAMPLE_DEFAULT, None) for lg in members],
                                          H, None, bbox, before, tb, avg_ptr, labels.data_ptr(), False, stream)

        got = {}
        for name, fn in (('resample + fnn_ensemble_export', two_step), ('fnn_ensemble_resample_export  ', fused)):
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats(dev)
            ms, lo, hi = _median_ms(fn, a.reps, dev)
            got[name] = (ms, labels.clone(), None if avg is None else avg[:, ::64].clone())
            lines.append(f'members {N}, {"labels + average" if with_avg else "labels only     "}, {name}: {ms:9.2f} ms  '
                         f'min {lo:.2f} max {hi:.2f}  peak {torch.cuda.max_memory_allocated(dev) / 1e9:6.1f} GB')
        (ms2, l2, a2), (ms1, l1, a1) = got.values()
        same = torch.equal(l1, l2) and (a1 is None or torch.equal(a1.view(torch.int32), a2.view(torch.int32)))
        lines.append(f'members {N}: fused / two-step = {ms1 / ms2:.3f}; same labels{" and average (every 64th plane)" if with_avg else ""}: {same}')
        del avg, got, l1, l2, a1, a2
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=512)
    ap.add_argument('--heads', type=int, default=61)
    ap.add_argument('--members', type=int, nargs='+', default=[2, 5])
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--numpy-n', type=int, default=128)
    ap.add_argument('--out', default=None)
    ap.add_argument('--section', choices=('export', 'resample'), default='export')
    a = ap.parse_args()
    from fast_nnunet_amd import capi

    dev = torch.device('cuda', 0)
    if a.section == 'resample':
        text = '\n'.join(resample_section(a, capi, dev))
        print(text)
        if a.out:
            with open(a.out, 'w') as f:
                f.write(text + '\n')
        return
    stream = torch.cuda.current_stream(dev).cuda_stream
    n, H = a.n, a.heads
    vox = n ** 3
    bbox, before, tb = [[0, n]] * 3, (n, n, n), (0, 1, 2)
    lines = [f'ensemble_bench: {H} heads, {n}^3 raw grid = crop, fp16 logits per member',
             f'device {torch.cuda.get_device_name(dev)}; median of {a.reps} after one warm-up, CUDA events on the stream '
             f'(the call synchronises); GB/s = (logit bytes read once + label bytes + average bytes written) / time; '
             f'copy rate {COPY_TBS} TB/s']
    logits = []
    g = torch.Generator(device=dev).manual_seed(5)
    labels = torch.empty((n, n, n), dtype=torch.uint8, device=dev)
    for N in sorted(a.members):
        while len(logits) < N:
            logits.append((torch.randn((H, n, n, n), generator=g, device=dev, dtype=torch.half) * 3))
        ptrs = [t.data_ptr() for t in logits[:N]]
        for with_avg in (False, True):
            avg = torch.empty((H, n, n, n), dtype=torch.float32, device=dev) if with_avg else None
            ts = []
            for r in range(a.reps + 1):
                torch.cuda.synchronize(dev)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                capi.ensemble_export(ptrs, [True] * N, H, None, bbox, before, tb, None if avg is None else avg.data_ptr(),
                                     labels.data_ptr(), False, stream)
                e1.record()
                e1.synchronize()
                if r:
                    ts.append(e0.elapsed_time(e1))
            ms = float(np.median(ts))
            nbytes = N * H * vox * 2 + vox + (H * vox * 4 if with_avg else 0)
            gbs = nbytes / ms / 1e6
            lines.append(f'members {N}, {"labels + average" if with_avg else "labels only     "}: {ms:8.2f} ms  '
                         f'({nbytes / 1e9:6.1f} GB, {gbs:7.0f} GB/s = {100 * gbs / (COPY_TBS * 1e3):5.1f} % of copy rate)'
                         f'  min {min(ts):.2f} max {max(ts):.2f}')
            del avg
            torch.cuda.empty_cache()
    del logits
    torch.cuda.empty_cache()

    # the numpy route: each member's float32 probabilities on the host (what the .npz files hold), averaged and argmaxed
    m = a.numpy_n
    rng = np.random.default_rng(3)
    for N in sorted(a.members):
        probs = [rng.random((H, m, m, m), dtype=np.float32) for _ in range(N)]
        t0 = time.perf_counter()
        avg = probs[0].astype(np.float32)
        for p in probs[1:]:
            avg += p
        avg /= N
        seg = avg.argmax(0)
        dt = time.perf_counter() - t0
        lines.append(f'numpy route, members {N}, {H} x {m}^3 float32 already in host memory (no .npz read): '
                     f'{dt * 1e3:.1f} ms; x{(n / m) ** 3:.0f} voxels for {n}^3 = {dt * (n / m) ** 3:.1f} s extrapolated')
        del probs, avg, seg
    text = '\n'.join(lines)
    print(text)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
