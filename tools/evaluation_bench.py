"""Evaluation on one MI355X: the counting pass (fnn_confusion_counts) on a synthetic 512^3 61-label uint8 pair for 1 and
3 predictions, and determine_postprocessing per case over a handful of such cases, with the numpy restatement's seconds
on a smaller case next to them.

usage (repo root, GPU box): python tools/evaluation_bench.py [--n 512] [--cases 3] [--reps 10] [--out FILE]
Kernel times: run it under rocprofv3 --kernel-trace --stats.

--section surface: the surface-distance entries (fnn_surface_count, fnn_surface_distances) on a 61-label pair whose
prediction is the reference with perturbed boundaries, the scipy route for three labels on this machine's CPU, and
compute_metrics_on_folder with and without surface_metrics; writes profiles/r26_surface_metrics.txt unless --out names
another file.

--section instance: fnn_instance_overlaps on the same 60-ellipsoid pair and on a pair of 20000 small lesions - the call, its
three labellings against one fnn_keep_largest_components on the same map, the scipy route (two labellings + np.unique of the
paired ids) for one label on this machine's CPU, and compute_metrics_on_folder with and without instance_metrics; writes
profiles/r27_instance_metrics.txt unless --out names another file.
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


def organ_map(n, seed=61):
    """60 ellipsoids of labels 1..60 with semi-axes n/32 .. n/6 at random places (later ones paint over earlier ones): compact
    label boxes, as organs have."""
    rng = np.random.default_rng(seed)
    seg = np.zeros((n, n, n), np.uint8)
    for label in range(1, 61):
        radii = rng.integers(max(2, n // 32), max(3, n // 6), 3)
        centre = [int(rng.integers(r, n - r)) for r in radii]
        box = tuple(slice(c - r, c + r + 1) for c, r in zip(centre, radii))
        z, y, x = np.ogrid[tuple(slice(-int(r), int(r) + 1) for r in radii)]
        inside = (z / radii[0]) ** 2 + (y / radii[1]) ** 2 + (x / radii[2]) ** 2 <= 1.0
        seg[box][inside] = label
    return seg


def perturbed_boundaries(seg, seed):
    """The map with every boundary moved by one voxel along x inside about half of its 16^3 blocks."""
    rng = np.random.default_rng(seed)
    blocks = rng.random(tuple((n + 15) // 16 for n in seg.shape)) < 0.5
    where = np.repeat(np.repeat(np.repeat(blocks, 16, 0), 16, 1), 16, 2)[:seg.shape[0], :seg.shape[1], :seg.shape[2]]
    moved = np.roll(seg, 1, axis=2)
    moved[:, :, 0] = seg[:, :, 0]
    return np.where(where, moved, seg)


def _events(dev, fn, reps):
    ts = []
    for r in range(reps + 1):
        torch.cuda.synchronize(dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize(dev)
        if r:
            ts.append(e0.elapsed_time(e1))
    return float(np.median(ts)), min(ts), max(ts), out


def surface_section(a):
    import tempfile
    from scipy import ndimage as ndi
    from fast_nnunet_amd import capi
    from fast_nnunet_amd import evaluation as ev
    from fast_nnunet_amd.imageio import NiftiIO
    dev = torch.device('cuda', 0)
    spacing = (2.5, 0.7421875, 0.7421875)
    labels = list(range(1, 61))
    ref = organ_map(a.n)
    pred = perturbed_boundaries(ref, 7)
    member = ev.region_members(labels)
    d_ref, d_pred = torch.from_numpy(ref).to(dev).reshape(-1), torch.from_numpy(pred).to(dev).reshape(-1)
    stream = torch.cuda.current_stream(dev).cuda_stream
    lines = [f'evaluation_bench --section surface: {a.n}^3 uint8 pair, 61 labels (60 ellipsoids measured, organ_map), prediction = reference with '
             f'boundaries moved by one voxel in half of the 16^3 blocks; {int((ref != pred).sum())} voxels differ; spacing {spacing}; '
             f'device {torch.cuda.get_device_name(dev)}',
             f'device calls: median (min, max) of {a.reps} after one warm-up, events around the call (scratch allocation, '
             f'launches and the synchronising copy-back of the sizes included)']
    ms, lo, hi, (n_surface, boxes) = _events(
        dev, lambda: capi.surface_count(d_ref.data_ptr(), d_pred.data_ptr(), False, ref.shape, member, stream), a.reps)
    lines.append(f'fnn_surface_count, 60 regions: {ms:.2f} ms (min {lo:.2f} max {hi:.2f})')
    both = (n_surface[:, 0] > 0) & (n_surface[:, 1] > 0)
    total = int(n_surface[both].sum())
    volumes = np.prod(boxes[:, 1::2] - boxes[:, 0::2], axis=1)
    buf = torch.empty(max(total, 1), dtype=torch.float64, device=dev)
    ms, lo, hi, _ = _events(dev, lambda: capi.surface_distances(d_ref.data_ptr(), d_pred.data_ptr(), False, ref.shape, member, spacing,
                                                                buf.data_ptr(), total, stream), a.reps)
    lines.append(f'fnn_surface_distances, {int(both.sum())} regions with two sides, {total} distances: {ms:.2f} ms (min {lo:.2f} max '
                 f'{hi:.2f}); box voxels walked (both directions): {2 * int(volumes[both].sum())} = '
                 f'{2 * volumes[both].sum() / ref.size:.2f} volumes; largest box {int(volumes.max())} voxels '
                 f'({int(volumes.max()) * 12 / 2 ** 20:.0f} MiB of scratch)')
    t0 = time.perf_counter()
    host = buf[:total].cpu().numpy()
    lines.append(f'download of the distances: {total * 8 / 1e6:.1f} MB in {(time.perf_counter() - t0) * 1e3:.2f} ms')
    t0 = time.perf_counter()
    got = ev.compute_surface_metrics(d_ref.reshape(ref.shape), d_pred.reshape(ref.shape), labels, spacing, checked=True)
    lines.append(f'compute_surface_metrics (count, distances, download, numpy metrics of 60 labels): '
                 f'{(time.perf_counter() - t0) * 1e3:.1f} ms')

    # the scipy route on this machine's CPU for three labels, cropped to the same boxes and on the whole volume
    structure = ndi.generate_binary_structure(3, 1)

    def scipy_route(mr, mp):
        t = time.perf_counter()
        sr_, sp_ = mr & ~ndi.binary_erosion(mr, structure, border_value=0), mp & ~ndi.binary_erosion(mp, structure, border_value=0)
        dp = ndi.distance_transform_edt(~sr_, sampling=spacing)[sp_]
        dr = ndi.distance_transform_edt(~sp_, sampling=spacing)[sr_]
        return time.perf_counter() - t, dp, dr

    offsets = np.concatenate([[0], np.cumsum(np.where(both, n_surface.sum(1), 0))])
    picked = [int(k) for k in np.argsort(volumes)[[len(volumes) // 4, len(volumes) // 2, -1]] if both[k]]
    lines.append(f'scipy route (binary_erosion + distance_transform_edt + indexing, both directions) on this machine\'s CPU, '
                 f'labels {[labels[k] for k in picked]} (a small, the median and the largest box):')
    for n_done, k in enumerate(picked):
        z0, z1, y0, y1, x0, x1 = (int(v) for v in boxes[k])
        mr, mp = ref == labels[k], pred == labels[k]
        # a margin of one voxel keeps the faces of the crop off the mask where the volume goes on
        crop = (slice(max(z0 - 1, 0), z1 + 1), slice(max(y0 - 1, 0), y1 + 1), slice(max(x0 - 1, 0), x1 + 1))
        t_crop, dp, dr = scipy_route(mr[crop], mp[crop])
        mine = np.sqrt(host[offsets[k]:offsets[k + 1]])
        equal = np.array_equal(mine, np.concatenate([dp, dr]))
        close = equal or bool(np.allclose(mine, np.concatenate([dp, dr]), rtol=1e-12, atol=0))
        line = (f'  label {labels[k]}: box {z1 - z0} x {y1 - y0} x {x1 - x0}, {len(mine)} distances; cropped {t_crop:.2f} s; '
                f'device values equal scipy\'s bit for bit: {equal} (within rtol 1e-12: {close})')
        if n_done < a.uncropped_labels:
            t_full, dp_f, dr_f = scipy_route(mr, mp)
            line += f'; uncropped {t_full:.1f} s, same values: {np.array_equal(dp_f, dp) and np.array_equal(dr_f, dr)}'
        lines.append(line)
        print(line, flush=True)

    # the folder command with and without the flag
    rw = NiftiIO()
    with tempfile.TemporaryDirectory() as tmp:
        fr, fp = os.path.join(tmp, 'ref'), os.path.join(tmp, 'pred')
        os.makedirs(fr), os.makedirs(fp)
        affine = np.diag([spacing[2], spacing[1], spacing[0], 1.0])
        for c in range(a.cases):
            r = ref if c == 0 else organ_map(a.n, seed=62 + c)
            rw.write_seg(r, os.path.join(fr, f'case{c}.nii.gz'), {'nibabel_stuff': {'original_affine': affine}})
            rw.write_seg(perturbed_boundaries(r, 7 + c), os.path.join(fp, f'case{c}.nii.gz'), {'nibabel_stuff': {'original_affine': affine}})
        for flag in (False, True):
            ev.compute_metrics_on_folder(fr, fp, None, rw, '.nii.gz', labels, surface_metrics=flag)        # warm-up
            t0 = time.perf_counter()
            summary = ev.compute_metrics_on_folder(fr, fp, None, rw, '.nii.gz', labels, surface_metrics=flag)
            t = time.perf_counter() - t0
            lines.append(f'compute_metrics_on_folder, {a.cases} cases of {a.n}^3 (files written by zlib, inflated on the host), '
                         f'surface_metrics={flag}: {t / a.cases * 1e3:.0f} ms per case; keys per label {len(summary["mean"][1])}')
    lines.append(f'label 1 of case 0: HD {got[1]["HD"]:.4f} HD95 {got[1]["HD95"]:.4f} ASSD {got[1]["ASSD"]:.4f} NSD {got[1]["NSD"]:.4f}')
    text = '\n'.join(lines)
    print(text)
    out = a.out or os.path.join(ROOT, 'profiles', 'r26_surface_metrics.txt')
    with open(out, 'w') as fh:
        fh.write(text + '\n')


def lesion_map(n, seed=27, lesions=20000, keep=1.0, extra=0):
    """``lesions`` ellipsoids of label 1 with semi-axes 1..3 at random places: many small components.  ``keep`` < 1 leaves a
    random part of them out and ``extra`` adds others (a prediction with misses and false positives); the same seed places
    the same lesions."""
    rng = np.random.default_rng(seed)
    centres, radii = rng.integers(4, n - 4, (lesions, 3)), rng.integers(1, 4, (lesions, 3))
    pick = np.random.default_rng(seed + 1)
    kept = pick.random(lesions) < keep
    centres = np.concatenate([centres[kept], pick.integers(4, n - 4, (extra, 3))])
    radii = np.concatenate([radii[kept], pick.integers(1, 4, (extra, 3))])
    seg = np.zeros((n, n, n), np.uint8)
    for c, r in zip(centres, radii):
        z, y, x = np.ogrid[tuple(slice(-int(v), int(v) + 1) for v in r)]
        inside = (z / r[0]) ** 2 + (y / r[1]) ** 2 + (x / r[2]) ** 2 <= 1.0
        seg[tuple(slice(int(a - b), int(a + b) + 1) for a, b in zip(c, r))][inside] = 1
    return seg


def instance_section(a):
    import tempfile
    from scipy import ndimage as ndi
    from fast_nnunet_amd import capi
    from fast_nnunet_amd import evaluation as ev
    from fast_nnunet_amd.imageio import NiftiIO
    dev = torch.device('cuda', 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    organs = organ_map(a.n)
    lesions = lesion_map(a.n)
    maps = {'organs': (organs, perturbed_boundaries(organs, 7), list(range(1, 61))),
            'lesions': (lesions, np.roll(lesion_map(a.n, keep=0.8, extra=2000), 1, axis=2), [1])}
    lines = [f'evaluation_bench --section instance: {a.n}^3 uint8 pairs; device {torch.cuda.get_device_name(dev)}',
             '  organs: 60 ellipsoids (organ_map), prediction = reference with boundaries moved by one voxel in half of the 16^3 blocks',
             '  lesions: 20000 ellipsoids of label 1 with semi-axes 1..3 (lesion_map), prediction = 80 % of them and 2000 others, '
             'rolled by one voxel along x',
             f'device calls: median (min, max) of {a.reps} after one warm-up, events around the call (scratch allocation, launches '
             f'and the synchronising copy-back of the counts included)']
    full = np.ones((3, 3, 3), int)
    for name, (ref, pred, labels) in maps.items():
        table = np.full(max(labels) + 1, -1, np.int32)
        table[labels] = np.arange(len(labels))
        d_ref, d_pred = torch.from_numpy(ref).to(dev), torch.from_numpy(pred).to(dev)
        probe = torch.empty(3, dtype=torch.int32, device=dev)
        n_out = capi.instance_overlaps_call(d_ref.data_ptr(), d_pred.data_ptr(), False, ref.shape, table, len(labels),
                                            probe.data_ptr(), 0, stream)
        total = int(n_out.sum())
        buf = torch.empty(max(total, 1) * 3, dtype=torch.int32, device=dev)
        lines.append(f'{name}: {len(labels)} label(s); foreground voxels {int((ref > 0).sum())} / {int((pred > 0).sum())}; components '
                     f'{int(n_out[0])} ref, {int(n_out[1])} pred, {int(n_out[2])} pieces')
        for what, cap in (('records written', total), ('cap 0: the labellings and the counts only', 0)):
            ms, lo, hi, _ = _events(dev, lambda: capi.instance_overlaps_call(d_ref.data_ptr(), d_pred.data_ptr(), False, ref.shape, table,
                                                                             len(labels), buf.data_ptr(), cap, stream), a.reps)
            lines.append(f'  fnn_instance_overlaps, {what}: {ms:.2f} ms (min {lo:.2f} max {hi:.2f})')
        ts = []
        for r in range(a.reps + 1):
            work = d_ref.clone()
            torch.cuda.synchronize(dev)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            capi.keep_largest_components(work.data_ptr(), False, ref.shape, table, len(labels), 0, stream)
            e1.record()
            torch.cuda.synchronize(dev)
            if r:
                ts.append(e0.elapsed_time(e1))
        lines.append(f'  one fnn_keep_largest_components on the reference map (one labelling, same sets): {np.median(ts):.2f} ms (min '
                     f'{min(ts):.2f} max {max(ts):.2f})')
        t0 = time.perf_counter()
        got = ev.compute_instance_metrics(d_ref, d_pred, labels, checked=True)
        lines.append(f'  compute_instance_metrics (call, download of {total * 12 / 1e6:.2f} MB, numpy merge and metrics of {len(labels)} '
                     f'label(s)): {(time.perf_counter() - t0) * 1e3:.1f} ms')
        # the host route on this machine's CPU for one label: two labellings and the unique pairs
        label = labels[len(labels) // 2]
        t0 = time.perf_counter()
        ids_r, n_r = ndi.label(ref == label, full)
        ids_p, n_p = ndi.label(pred == label, full)
        both = (ids_r > 0) & (ids_p > 0)
        key, count = np.unique(ids_p[both].astype(np.int64) * (n_r + 1) + ids_r[both], return_counts=True)
        t_host = time.perf_counter() - t0
        mine = ev.instance_overlaps(d_ref, d_pred, [label], checked=True)[label]
        same = (len(mine['ref_sizes']) == n_r and len(mine['pred_sizes']) == n_p and
                np.array_equal(mine['pairs'][:, 2], count) and
                np.array_equal(mine['pairs'][:, 0] * (n_r + 1) + mine['pairs'][:, 1], key - (n_r + 1) - 1))
        lines.append(f'  host route for label {label} alone (scipy.ndimage.label with the full structure on both masks + np.unique of the '
                     f'paired ids) on this machine\'s CPU: {t_host:.2f} s; {n_r} / {n_p} components, {len(key)} pairs; the device\'s lists '
                     f'are the same: {same}')
        m = got[label]
        lines.append(f'  label {label}: inst_F1 {m["inst_F1"]:.4f} recall {m["inst_recall"]:.4f} precision {m["inst_precision"]:.4f} '
                     f'FN_inst_vox {m["FN_inst_vox"]} FP_inst_vox {m["FP_inst_vox"]} PQ {m["PQ"]:.4f} SQ {m["SQ"]:.4f} RQ {m["RQ"]:.4f}')
        print('\n'.join(lines[-7:]), flush=True)

    # the folder command with and without the flag
    rw = NiftiIO()
    props = {'nibabel_stuff': {'original_affine': np.eye(4)}}
    for name, (ref, pred, labels) in maps.items():
        with tempfile.TemporaryDirectory() as tmp:
            fr, fp = os.path.join(tmp, 'ref'), os.path.join(tmp, 'pred')
            os.makedirs(fr), os.makedirs(fp)
            for c in range(a.cases):
                rw.write_seg(np.roll(ref, 3 * c, axis=0), os.path.join(fr, f'case{c}.nii.gz'), props)
                rw.write_seg(np.roll(pred, 3 * c, axis=0), os.path.join(fp, f'case{c}.nii.gz'), props)
            for flag in (False, True):
                ev.compute_metrics_on_folder(fr, fp, None, rw, '.nii.gz', labels, instance_metrics=flag)        # warm-up
                t0 = time.perf_counter()
                summary = ev.compute_metrics_on_folder(fr, fp, None, rw, '.nii.gz', labels, instance_metrics=flag)
                t = time.perf_counter() - t0
                lines.append(f'compute_metrics_on_folder, {name}, {a.cases} cases of {a.n}^3 (files written by zlib, inflated on the host), '
                             f'instance_metrics={flag}: {t / a.cases * 1e3:.0f} ms per case; keys per label {len(summary["mean"][labels[0]])}')
    text = '\n'.join(lines)
    print(text)
    out = a.out or os.path.join(ROOT, 'profiles', 'r27_instance_metrics.txt')
    with open(out, 'w') as fh:
        fh.write(text + '\n')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--section', choices=('counts', 'surface', 'instance'), default='counts')
    ap.add_argument('--uncropped-labels', type=int, default=3, help='surface: of the three scipy labels, how many also run uncropped')
    ap.add_argument('--n', type=int, default=512)
    ap.add_argument('--cases', type=int, default=3)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--cpu-n', type=int, default=192)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if a.section == 'surface':
        return surface_section(a)
    if a.section == 'instance':
        return instance_section(a)
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
