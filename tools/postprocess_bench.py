"""Connected-component postprocessing on one MI355X: ms per pass and per pkl for a synthetic 512^3 61-label map (a
whole-foreground step plus one step per label, the shape of a typical postprocessing.pkl of a 61-class model), with
the scipy restatement's seconds on the host next to it.

usage (repo root, GPU box): python tools/postprocess_bench.py [--n 512] [--reps 5] [--no-cpu] [--out FILE]
Kernel times: run it under rocprofv3 --kernel-trace --stats.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch
from scipy import ndimage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def make_map(n, seed=61):
    rng = np.random.default_rng(seed)
    small = ndimage.gaussian_filter(rng.standard_normal((n // 8,) * 3).astype(np.float32), 1.0)
    field = ndimage.zoom(small, 8, order=1)
    seg = np.clip((field - 0.1) * 150, 0, 60).astype(np.uint8)
    seg[(field > 0.1) & (seg == 0)] = 1
    idx = rng.integers(0, seg.size, 20000)
    seg.reshape(-1)[idx] = rng.integers(1, 61, idx.size).astype(np.uint8)
    return seg


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=512)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--no-cpu', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    from fast_nnunet_amd import capi
    from fast_nnunet_amd import postprocessing as pp

    seg = make_map(a.n)
    labels = list(range(1, 61))
    f = pp.remove_all_but_largest_component_from_segmentation
    kwargs = [{'labels_or_regions': labels}] + [{'labels_or_regions': i} for i in labels]
    passes = pp.plan_passes([f] * len(kwargs), kwargs)
    dev = torch.device('cuda', 0)
    base = torch.from_numpy(seg).to(dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    lines = [f'postprocess_bench: {a.n}^3 uint8 map, {len(kwargs)} steps (whole foreground + {len(labels)} labels) '
             f'-> {len(passes)} passes; foreground voxels {int((seg > 0).sum())}',
             f'device {torch.cuda.get_device_name(dev)}; median of {a.reps} after one warm-up, CUDA events on the stream']

    def timed(fn):
        ts = []
        for r in range(a.reps + 1):
            work = base.clone()
            torch.cuda.synchronize(dev)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn(work)
            e1.record()
            torch.cuda.synchronize(dev)
            if r:
                ts.append(e0.elapsed_time(e1))
        return float(np.median(ts)), work if out is None else out

    for k, (_, body) in enumerate(passes):
        sets = [s for s, _, _ in body]
        table = np.full(61, -1, np.int32)
        for g, s in enumerate(sets):
            for v in s:
                table[v] = g
        ms, _ = timed(lambda w: capi.keep_largest_components(w.data_ptr(), False, w.shape, table, len(sets), 0, stream))
        lines.append(f'pass {k}: {len(sets)} set(s) in one labelling: {ms:.2f} ms (fnn_keep_largest_components, '
                     f'scratch allocation included)')
    ms, got = timed(lambda w: pp.apply_postprocessing(w, [f] * len(kwargs), kwargs))
    lines.append(f'pkl ({len(kwargs)} steps, {len(passes)} passes) through apply_postprocessing on a device tensor: {ms:.2f} ms')
    if not a.no_cpu:
        from test_postprocessing_cpu import keep_largest_ref, keep_largest_ref_boxed
        t0 = time.perf_counter()
        want = keep_largest_ref(seg, labels)
        t1 = time.perf_counter()
        boxes = ndimage.find_objects(want)
        for lab in labels:
            if lab - 1 < len(boxes) and boxes[lab - 1] is not None:
                want = keep_largest_ref_boxed(want, lab, 0, boxes[lab - 1])
        t2 = time.perf_counter()
        ok = np.array_equal(got.cpu().numpy(), want)
        lines.append(f'CPU restatement (scipy ndimage.label, one thread): whole-foreground step {t1 - t0:.2f} s, '
                     f'{len(labels)} per-label steps in their find_objects boxes {t2 - t1:.2f} s; '
                     f'device result bit-identical: {ok}')
    text = '\n'.join(lines)
    print(text)
    if a.out:
        with open(a.out, 'w') as fh:
            fh.write(text + '\n')


if __name__ == '__main__':
    main()
