"""Connected-component postprocessing on one MI355X: ms per pass and per pkl for a synthetic 512^3 61-label map (a
whole-foreground step plus one step per label, the shape of a typical postprocessing.pkl of a 61-class model), with
the scipy restatement's seconds on the host next to it.

usage (repo root, GPU box): python tools/postprocess_bench.py [--n 512] [--reps 5] [--no-cpu] [--out FILE] [--section NAME]
Kernel times: run it under rocprofv3 --kernel-trace --stats.

--section small_holes (profiles/r33_small_holes.txt): fnn_remove_small_components and fnn_fill_holes on evaluation_bench's two
maps - 60 ellipsoids with cavities punched into them, and 20000 small lesions - next to fnn_keep_largest_components on the same
map in the same run and to scipy on this machine's CPU (ndimage.label + bincount, binary_fill_holes in the label's box).

--section morphology (profiles/r34_morphology.txt): fnn_binary_morphology on the same two maps - dilate, erode, open and close
at connectivity 6 and 26 with 1, 2, 5 and 10 iterations, one call per label and one call for the whole foreground as a region,
next to scipy on this machine's CPU per label cropped to the label's box (--cpu-n: the iteration counts scipy runs for).
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


def punch_cavities(seg):
    """A closed cavity (an ellipsoid of background, a third of the box's half-extents) at the centre of every label's box,
    where the label itself lies there: holes for fnn_fill_holes to find.  Where another ellipsoid was painted over the
    centre the label keeps no cavity."""
    out = seg.copy()
    for lab, box in enumerate(ndimage.find_objects(seg), 1):
        if box is None:
            continue
        half = [max(1, (s.stop - s.start) // 6) for s in box]
        centre = [(s.start + s.stop) // 2 for s in box]
        z, y, x = np.ogrid[tuple(slice(-h, h + 1) for h in half)]
        inside = (z / half[0]) ** 2 + (y / half[1]) ** 2 + (x / half[2]) ** 2 <= 1.0
        sub = out[tuple(slice(c - h, c + h + 1) for c, h in zip(centre, half))]
        sub[inside & (sub == lab)] = 0
    return out


def small_holes_section(a):
    """fnn_remove_small_components (all sets in one call) and fnn_fill_holes (one call per label) against
    fnn_keep_largest_components on the same map and scipy on the host."""
    from fast_nnunet_amd import capi
    from tools.evaluation_bench import lesion_map, organ_map
    import pp_morph_ref as ref
    dev = torch.device('cuda', 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    maps = {'organs': (punch_cavities(organ_map(a.n)), list(range(1, 61)), 50),
            'lesions': (lesion_map(a.n), [1], 20)}
    lines = [f'postprocess_bench --section small_holes: {a.n}^3 uint8 maps; device {torch.cuda.get_device_name(dev)}',
             '  organs: 60 ellipsoids (evaluation_bench.organ_map) with an ellipsoidal cavity punched into the centre of each label box',
             '  lesions: 20000 ellipsoids of label 1 with semi-axes 1..3 (evaluation_bench.lesion_map)',
             f'device calls: median (min, max) of {a.reps} after one warm-up, events around the call on a fresh copy of the map (scratch '
             f'allocation, launches and the synchronising copy-back of the counts included)']

    def report(text):
        lines.append(text)
        print(text, flush=True)
    for text in lines:
        print(text, flush=True)

    for name, (seg, labels, min_size) in maps.items():
        table = np.full(max(labels) + 1, -1, np.int32)
        table[labels] = np.arange(len(labels))
        base = torch.from_numpy(seg).to(dev)
        report(f'{name}: {len(labels)} label(s), foreground voxels {int((seg > 0).sum())}')

        def timed(fn):
            ts = []
            for r in range(a.reps + 1):
                w = base.clone()
                torch.cuda.synchronize(dev)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                out = fn(w)
                e1.record()
                torch.cuda.synchronize(dev)
                if r:
                    ts.append(e0.elapsed_time(e1))
            return float(np.median(ts)), min(ts), max(ts), w, out
        ms, lo, hi, _, _ = timed(lambda w: capi.keep_largest_components(w.data_ptr(), False, w.shape, table, len(labels), 0, stream))
        report(f'  fnn_keep_largest_components, all {len(labels)} set(s) in one labelling: {ms:.2f} ms (min {lo:.2f} max {hi:.2f})')
        small = {}
        for conn in (26, 6):
            ms, lo, hi, w, removed = timed(lambda w: capi.remove_small_components(w.data_ptr(), False, w.shape, table, len(labels), 0,
                                                                                  [min_size] * len(labels), conn, stream))
            small[conn] = w.cpu().numpy()
            report(f'  fnn_remove_small_components, all {len(labels)} set(s), min_size {min_size}, connectivity {conn}: {ms:.2f} ms '
                   f'(min {lo:.2f} max {hi:.2f}); voxels removed {int(removed.sum())}')
        per_label, filled_total = [], 0
        w = base.clone()
        in_set = np.full(max(labels) + 1, -1, np.int32)
        for lab in labels:
            in_set[:] = -1
            in_set[lab] = 0
            ts = []
            for r in range(a.reps + 1):
                w.copy_(base)
                torch.cuda.synchronize(dev)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                n_filled = capi.fill_holes(w.data_ptr(), False, w.shape, in_set, 0, lab, 7, stream)
                e1.record()
                torch.cuda.synchronize(dev)
                if r:
                    ts.append(e0.elapsed_time(e1))
            per_label.append(float(np.median(ts)))
            filled_total += n_filled
        report(f'  fnn_fill_holes, one call per label: {sum(per_label):.2f} ms for {len(labels)} label(s) (sum of the per-label medians); per '
               f'label median {np.median(per_label):.2f} ms, min {min(per_label):.2f}, max {max(per_label):.2f}; voxels filled {filled_total}')
        w.copy_(base)
        t0 = time.perf_counter()
        for lab in labels:
            in_set[:] = -1
            in_set[lab] = 0
            capi.fill_holes(w.data_ptr(), False, w.shape, in_set, 0, lab, 7, stream)
        torch.cuda.synchronize(dev)
        report(f'  the same {len(labels)} call(s) one after another on one map, host clock: {(time.perf_counter() - t0) * 1e3:.2f} ms')
        holes_dev = w.cpu().numpy()
        if a.no_cpu:
            continue
        boxes = ndimage.find_objects(seg) if len(labels) > 1 else [tuple(slice(0, n) for n in seg.shape)]
        for conn in (26, 6):
            t0 = time.perf_counter()
            want = seg.copy()
            for lab in labels:
                box = boxes[lab - 1]
                if box is not None:
                    want[box][ref.small_components_of_set(seg[box], [lab], min_size, conn)] = 0
            report(f'  scipy ndimage.label + bincount, connectivity {conn}, per label in its find_objects box (one thread): '
                   f'{time.perf_counter() - t0:.2f} s; device result bit-identical: {np.array_equal(small[conn], want)}')
        t0 = time.perf_counter()
        want = seg.copy()
        for lab in labels:
            box = ndimage.find_objects((seg == lab).astype(np.uint8))[0] if len(labels) == 1 else boxes[lab - 1]
            if box is not None:
                sub = want[box]
                sub[ref.holes_of(seg[box] == lab) & (sub == 0)] = lab
        report(f'  scipy binary_fill_holes, per label cropped to its box (one thread): {time.perf_counter() - t0:.2f} s; device result '
               f'bit-identical: {np.array_equal(holes_dev, want)}')
    if a.out:
        with open(a.out, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


def morphology_section(a):
    """fnn_binary_morphology: one call per label, one call for the whole foreground, and scipy per label in the label's box."""
    from fast_nnunet_amd import capi
    from tools.evaluation_bench import lesion_map, organ_map
    import morph_ref as ref
    dev = torch.device('cuda', 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    maps = {'organs': (organ_map(a.n), list(range(1, 61))), 'lesions': (lesion_map(a.n), [1])}
    ops = [('dilation', capi.FNN_MORPH_DILATE), ('erosion', capi.FNN_MORPH_ERODE), ('opening', capi.FNN_MORPH_OPEN),
           ('closing', capi.FNN_MORPH_CLOSE)]
    cpu_n = [] if a.no_cpu else [int(v) for v in a.cpu_n.split(',') if v]
    lines = []

    def report(text):
        lines.append(text)
        print(text, flush=True)
    report(f'postprocess_bench --section morphology: {a.n}^3 uint8 maps; device {torch.cuda.get_device_name(dev)}')
    report('  organs: 60 ellipsoids (evaluation_bench.organ_map); lesions: 20000 ellipsoids of label 1 with semi-axes 1..3 (evaluation_bench.lesion_map)')
    report(f'device calls: median (min, max) of {a.reps} after one warm-up, events around the call on a fresh copy of the map (the box pass and '
           f'its host read, scratch allocation, one launch per iteration and the synchronising copy-back of the count included); border_value 0')
    report('  per label: one call per label, the sum of the per-label medians, and the median, min and max over the labels')
    report('  region: one call with every foreground label in the set (fill_label 1)')
    report('  scipy: one thread, per label on the crop of its find_objects box (grown by n for dilation and closing), in label order on one map;')
    report('  "same" says whether the device calls made in that order on one map give the same map, bit for bit')
    report('step kernel: one launch per iteration')

    def timed(base, w, fn):
        ts = []
        for r in range(a.reps + 1):
            w.copy_(base)
            torch.cuda.synchronize(dev)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn(w)
            e1.record()
            torch.cuda.synchronize(dev)
            if r:
                ts.append(e0.elapsed_time(e1))
        return float(np.median(ts)), min(ts), max(ts)

    for name, (seg, labels) in maps.items():
        base = torch.from_numpy(seg).to(dev)
        w = base.clone()
        boxes = ndimage.find_objects(seg)
        report(f'{name}: {len(labels)} label(s), foreground voxels {int((seg > 0).sum())}')
        region = np.full(max(labels) + 1, -1, np.int32)
        region[labels] = 0
        in_set = np.full(max(labels) + 1, -1, np.int32)
        for op, code in ops:
            for conn in (6, 26):
                for n in (1, 2, 5, 10):
                    per_label = []
                    for lab in labels:
                        in_set[:] = -1
                        in_set[lab] = 0
                        per_label.append(timed(base, w, lambda w: capi.binary_morphology(w.data_ptr(), False, w.shape, in_set, code, conn, n, 0,
                                                                                         0, lab, 7, stream))[0])
                    ms, lo, hi = timed(base, w, lambda w: capi.binary_morphology(w.data_ptr(), False, w.shape, region, code, conn, n, 0, 0, 1, 7,
                                                                                 stream))
                    text = (f'  {op:8s} connectivity {conn:2d} n {n:2d}: per label {sum(per_label):8.2f} ms (median {np.median(per_label):.3f}, min '
                            f'{min(per_label):.3f}, max {max(per_label):.3f}); region {ms:7.2f} ms (min {lo:.2f} max {hi:.2f})')
                    if n in cpu_n:
                        w.copy_(base)
                        changed = 0
                        for lab in labels:
                            in_set[:] = -1
                            in_set[lab] = 0
                            changed += capi.binary_morphology(w.data_ptr(), False, w.shape, in_set, code, conn, n, 0, 0, lab, 7, stream)
                        got = w.cpu().numpy()
                        grow = n if op in ref.ADDS else 0
                        want = seg.copy()
                        t0 = time.perf_counter()
                        for lab in labels:
                            if lab - 1 >= len(boxes) or boxes[lab - 1] is None:
                                continue
                            box = tuple(slice(max(0, s.start - grow), min(d, s.stop + grow)) for s, d in zip(boxes[lab - 1], seg.shape))
                            kw = dict(labels_or_regions=lab, iterations=n, connectivity=conn, border_value=0)
                            want[box] = ref.morph_ref(want[box], op, **kw)
                        text += f'; scipy {time.perf_counter() - t0:6.2f} s, same {np.array_equal(got, want)}, voxels written {changed}'
                    report(text)
    if a.out:
        with open(a.out, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=512)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--no-cpu', action='store_true')
    ap.add_argument('--out', default=None)
    ap.add_argument('--section', default='largest', choices=['largest', 'small_holes', 'morphology'])
    ap.add_argument('--cpu-n', default='1,2,5,10', help='--section morphology: the iteration counts scipy runs for (comma-separated)')
    a = ap.parse_args()
    if a.section == 'small_holes':
        return small_holes_section(a)
    if a.section == 'morphology':
        return morphology_section(a)
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
