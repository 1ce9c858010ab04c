"""Surface models on one MI355X: fnn_mesh_count and fnn_mesh_emit on two 512^3 uint8 label maps - the 60-ellipsoid organ
map and the 20000-small-lesion map of tools/evaluation_bench.py - with 0 and 25 smoothing pairs, a device copy of the output
bytes as the floor, the download of the payload, and the numpy route of tests/mesh_ref.py for one label cropped to its box
on this machine's CPU.  Writes profiles/r29_mesh.txt unless --out names another file.

With --decimate it measures fnn_mesh_decimate instead, on the same two maps with 0 and 25 smoothing pairs at the factors 0.2,
0.5 and 0.9: its time next to fnn_mesh_emit's for the same model, the rounds and the triangles before and after, the download
of the decimated payload against the full one, the numpy route of tests/mesh_decimate_ref.py for one organ, and the
compiler's registers and scratch of every kernel of csrc/mesh_decimate.hip.  Writes profiles/r30_mesh_decimate.txt.

usage (repo root, GPU box): python tools/mesh_bench.py [--decimate] [--n 512] [--calls 3] [--windows 5] [--out FILE]
Every device figure is the median (min, max) over --windows windows of one pair of events around --calls calls, divided by
the calls, after one warm-up window; a call includes its scratch allocation, its launches and its synchronising copy-backs."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from tools.evaluation_bench import lesion_map, organ_map  # noqa: E402


def windows(dev, fn, calls, n_windows):
    ts = []
    for w in range(n_windows + 1):
        torch.cuda.synchronize(dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        torch.cuda.synchronize(dev)
        if w:
            ts.append(e0.elapsed_time(e1) / calls)
    return f'{np.median(ts):.2f} ms (min {min(ts):.2f} max {max(ts):.2f})'


def kernel_resources(name):
    """The compiler's report next to csrc/<name>.o: one line per kernel with its registers, scratch and LDS."""
    import re
    path = os.path.join(ROOT, 'fast-nnunet_amd', 'csrc', name + '.res')
    if not os.path.isfile(path):
        return [f'  (no {name}.res next to the library: build with make to get the per-kernel resources)']
    out, cur = [], None
    for line in open(path):
        m = re.search(r'remark:\s+(Function Name|VGPRs|TotalSGPRs|ScratchSize \[bytes/lane\]|LDS Size \[bytes/block\]|Occupancy \[waves/SIMD\]): (.+?) \[-Rpass', line)
        if not m:
            continue
        if m.group(1) == 'Function Name':
            short = re.search(r'\d+([a-z]+_\w+?_kernel)', m.group(2))
            cur = {'name': short.group(1) if short else m.group(2)}
            out.append(cur)
        elif cur is not None:
            cur[m.group(1).split(' ')[0]] = m.group(2)
    return [f"  {k['name']:22s} VGPRs {k.get('VGPRs', '?'):>3s}  SGPRs {k.get('TotalSGPRs', '?'):>3s}  scratch {k.get('ScratchSize', '?')} B/lane  LDS {k.get('LDS', '?'):>4s} B  "
            f"occupancy {k.get('Occupancy', '?')} waves/SIMD" for k in out]


def decimate_section(a, dev, stream, maps, affine):
    import mesh_decimate_ref as dr
    import mesh_ref as mr
    from fast_nnunet_amd import capi, meshing
    lines = [f'mesh_bench --decimate: fnn_mesh_decimate on {a.n}^3 uint8 label maps (organs: 60 ellipsoids, one region per label; lesions: 20000 small '
             f'ellipsoids, one region), layout-0 model in, layout-1 (VTK payload) out; device {torch.cuda.get_device_name(dev)}',
             f'device figures: median (min, max) over {a.windows} windows of one event pair around {a.calls} calls (fnn_mesh_decimate: one call), per '
             f'call, after one warm-up window; a call includes its scratch allocation (144 B per point + 95 B per triangle), launches and '
             f'synchronising copy-backs']
    for name, (seg, labels) in maps.items():
        regions = [(v,) for v in labels]
        member = meshing._member_table(regions)
        d = torch.from_numpy(seg).to(dev)
        counts, boxes = capi.mesh_count(d.data_ptr(), False, seg.shape, member, stream)
        n, t = int(counts[:, 0].sum()), int(2 * counts[:, 1].sum())
        offsets = np.concatenate([[0], np.cumsum(counts[:, 0])]).astype(np.int64)
        lines.append(f'{name}: {len(regions)} region(s), {n} points, {t} triangles')
        pts, cells, reg = (torch.empty(max(k, 1), dtype=torch.uint8, device=dev) for k in (n * 12, t * 12, t * 2))
        out = [torch.empty(max(k, 1), dtype=torch.uint8, device=dev) for k in (n * 12, t * 16, t * 2)]
        host = [torch.empty(x.shape, dtype=torch.uint8).pin_memory() for x in out]
        for pairs in (0, 25):
            def emit():
                capi.mesh_emit(d.data_ptr(), False, seg.shape, member, affine, pairs, 0, pts.data_ptr(), n, cells.data_ptr(), t, reg.data_ptr(), stream)
            lines.append(f'  {pairs} smoothing pairs: fnn_mesh_emit, layout 0: {windows(dev, emit, a.calls, a.windows)}')

            def download(sizes):
                for h, x, k in zip(host, out, sizes):
                    h[:k].copy_(x[:k], non_blocking=True)
                torch.cuda.synchronize(dev)
            full = (n * 12, t * 16, t * 2)
            lines.append(f'    download of the full layout-1 payload ({sum(full) / 1e6:.1f} MB) into pinned memory: '
                         f'{windows(dev, lambda: download(full), a.calls, a.windows)}')
            for factor in (0.2, 0.5, 0.9):
                res = []

                def decimate():
                    res[:] = capi.mesh_decimate(pts.data_ptr(), n, cells.data_ptr(), reg.data_ptr(), t, offsets, factor, 1, out[0].data_ptr(), n,
                                                out[1].data_ptr(), t, out[2].data_ptr(), stream)
                timing = windows(dev, decimate, 1, a.windows)
                _, n_out, t_out, rounds, exhausted = res
                small = (n_out * 12, t_out * 16, t_out * 2)
                lines.append(f'    d = {factor}: fnn_mesh_decimate {timing}; {rounds} rounds, {t} -> {t_out} triangles (target {int(np.ceil((1.0 - factor) * t))}), '
                             f'{n} -> {n_out} points, exhausted {exhausted}')
                lines.append(f'      download of the decimated payload ({sum(small) / 1e6:.1f} MB): {windows(dev, lambda: download(small), a.calls, a.windows)}')
                print('\n'.join(lines[-2:]), flush=True)
        if name == 'organs':                                         # the host route for one organ cropped to its box
            r = int(np.argmax(counts[:, 0]))
            b = boxes[r]
            crop = np.pad((seg[b[0]:b[1], b[2]:b[3], b[4]:b[5]] == labels[r]).astype(np.uint8), 1)
            surface = mr.mesh(crop, [[1]], affine=affine)
            for factor in (0.2, 0.5):
                t0 = time.perf_counter()
                ref = dr.decimate_mesh(surface, factor)
                lines.append(f'  numpy (tests/mesh_decimate_ref.py) for label {labels[r]} alone, {len(surface["triangles"])} triangles, 0 pairs, d = {factor}: '
                             f'{time.perf_counter() - t0:.2f} s, {ref["rounds"]} rounds, {len(ref["triangles"])} triangles on this machine\'s CPU')
                print(lines[-1], flush=True)
    lines.append('kernels of csrc/mesh_decimate.hip as compiled for gfx950 (-Rpass-analysis=kernel-resource-usage):')
    return lines + kernel_resources('mesh_decimate')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--decimate', action='store_true', help='measure fnn_mesh_decimate (profiles/r30_mesh_decimate.txt)')
    ap.add_argument('--n', type=int, default=512)
    ap.add_argument('--calls', type=int, default=3)
    ap.add_argument('--windows', type=int, default=5)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    a.out = a.out or os.path.join(ROOT, 'profiles', 'r30_mesh_decimate.txt' if a.decimate else 'r29_mesh.txt')
    import mesh_ref as mr
    from fast_nnunet_amd import capi, meshing
    dev = torch.device('cuda', 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    affine = np.array([[0.7421875, 0, 0, -190.0], [0, 0.7421875, 0, -190.0], [0, 0, 2.5, -640.0], [0, 0, 0, 1]])
    maps = {'organs': (organ_map(a.n), list(range(1, 61))), 'lesions': (lesion_map(a.n), [1])}
    lines = [f'mesh_bench: {a.n}^3 uint8 label maps; organs: 60 ellipsoids of labels 1..60, one region per label (organ_map); lesions: 20000 '
             f'ellipsoids of label 1 with semi-axes 1..3, one region (lesion_map); anisotropic affine; device {torch.cuda.get_device_name(dev)}',
             f'device figures: median (min, max) over {a.windows} windows of one event pair around {a.calls} calls, per call, after one warm-up '
             f'window; a call includes its scratch allocation, launches and synchronising copy-backs']
    for name, (seg, labels) in ({} if a.decimate else maps).items():
        regions = [(v,) for v in labels]
        member = meshing._member_table(regions)
        d = torch.from_numpy(seg).to(dev)
        counts, boxes = capi.mesh_count(d.data_ptr(), False, seg.shape, member, stream)
        n, t = int(counts[:, 0].sum()), int(2 * counts[:, 1].sum())
        box_vox = int(np.prod(boxes[:, 1::2] - boxes[:, 0::2], axis=1).sum())
        lines.append(f'{name}: {len(regions)} region(s), {int((seg > 0).sum())} foreground voxels, {n} points, {t} triangles, the regions\' boxes hold '
                     f'{box_vox} voxels ({box_vox / seg.size:.2f} of the map)')
        lines.append(f'  fnn_mesh_count: {windows(dev, lambda: capi.mesh_count(d.data_ptr(), False, seg.shape, member, stream), a.calls, a.windows)}')
        for layout in (0, 1):
            pts = torch.empty(max(n, 1) * 12, dtype=torch.uint8, device=dev)
            cells = torch.empty(max(t, 1) * (16 if layout else 12), dtype=torch.uint8, device=dev)
            reg = torch.empty(max(t, 1) * 2, dtype=torch.uint8, device=dev)
            for pairs in (0, 25):
                def emit():
                    capi.mesh_emit(d.data_ptr(), False, seg.shape, member, affine, pairs, layout, pts.data_ptr(), n, cells.data_ptr(), t,
                                   reg.data_ptr(), stream)
                lines.append(f'  fnn_mesh_emit, layout {layout}, {pairs} smoothing pairs: {windows(dev, emit, a.calls, a.windows)}')
            total = pts.numel() + cells.numel() + reg.numel()
            src = torch.cat([pts, cells, reg])
            dst = torch.empty_like(src)
            lines.append(f'  layout {layout}: output {total / 1e6:.1f} MB; device copy of as many bytes (the floor): '
                         f'{windows(dev, lambda: dst.copy_(src), 20, a.windows)}')
            host = [torch.empty(x.shape, dtype=torch.uint8).pin_memory() for x in (pts, cells, reg)]

            def download():
                for h, x in zip(host, (pts, cells, reg)):
                    h.copy_(x, non_blocking=True)
                torch.cuda.synchronize(dev)
            lines.append(f'  layout {layout}: download of the payload into pinned memory: {windows(dev, download, a.calls, a.windows)}')
        # the host route for one label cropped to its box
        r = int(np.argmax(counts[:, 0]))
        b = boxes[r]
        crop = seg[b[0]:b[1], b[2]:b[3], b[4]:b[5]] == labels[r]
        t0 = time.perf_counter()
        corners, tri, nbr, _ = mr.region_topology(crop)
        topo = time.perf_counter() - t0
        for pairs in (0, 25):
            t0 = time.perf_counter()
            pos = mr.smooth(corners[:, ::-1].astype(np.float32) - np.float32(0.5), nbr, pairs)
            mr.to_world(pos, affine)
            lines.append(f'  numpy (tests/mesh_ref.py) for label {labels[r]} alone, cropped to its box {tuple(int(v) for v in crop.shape)}, {len(corners)} '
                         f'points, {pairs} pairs: {topo:.2f} s for faces, vertices and neighbours + {time.perf_counter() - t0:.2f} s for positions on '
                         f'this machine\'s CPU')
        print('\n'.join(lines[-12:]), flush=True)
    if a.decimate:
        lines = decimate_section(a, dev, stream, maps, affine)
    text = '\n'.join(lines) + '\n'
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
