"""Image files on one MI355X: what the route from a NIfTI file to the float32 [C, z, y, x] device tensor that
DevicePreprocessor.run_case_npy takes costs, split into its parts, next to the route a caller had before NiftiIO (host decode
with numpy, astype(float32), then predict_single_npy_array's upload of the float32 array); the decode kernel's rate next to
a plain device copy of the same bytes; the write of a label map; and predict_from_files (reader and writer threads)
against predict_from_files_sequential on four cases; and (``--section reorient`` runs these rows alone) fnn_reorient on an
n^3 case - float32 forward and uint8 backward, one orientation per kernel path - next to a device-to-device copy of the
same bytes and to numpy's flip / transpose on the host; and (``--section deflate``, these rows alone) fnn_deflate_labels on
a synthetic 61-label map of n^3 voxels as uint8 and uint16 and on the golden mask tiled to a similar size, next to a device
copy of the same bytes, to zlib level 1 on this machine's CPU, and the download of the fragment next to that of the map, and
fnn_deflate_labels_dyn (per-chunk dynamic Huffman tables) next to the fixed call in alternating windows, its fragment's size
next to zlib levels 1 and 6 and its download (profiles/r31_deflate_dynamic.txt); and
(``--section masks``, these rows alone) the per-label mask files of JHUPredictor: fnn_deflate_masks_count + fnn_deflate_masks_emit
on synthetic maps of 61 and 118 labels and on the golden mask tiled, next to one fnn_deflate_labels call per mask materialised on
the device, to zlib level 1 of a mask on the CPU times the number of labels, and the sizes that are downloaded and written; and
(``--section label_files``, these rows alone, written to profiles/r21_label_files.txt unless ``--out`` says otherwise)
fnn_decode_labels on the int16 and the uint8 bytes of an n^3 label map next to fnn_decode_voxels followed by the cast it
replaces and to a device copy of the same bytes, and compute_metrics_on_folder on a few generated cases of n^3 voxels, per
case and split into inflate, upload, decode and count; and (``--section inflate``, these rows alone, written to
profiles/r25_inflate.txt unless ``--out`` says otherwise) fnn_inflate_segments on the fragments fnn_deflate_labels makes of an
n^3 map - 61 labels as uint8 and uint16 (long runs) and a map without runs (every byte a literal) - and on the fragments of
60 masks, next to zlib's inflate of the same bytes on this machine's CPU and a device copy of the output, and
compute_metrics_on_folder and apply_postprocessing_to_folder per case with ``inflate_on_device`` off and on over predictions
written with ``compress_on_device=True``; and (``--section inflate_dyn``, these rows alone, written to
profiles/r32_inflate_dynamic.txt unless ``--out`` says otherwise) fnn_inflate_segments_dyn on the fragments
fnn_deflate_labels_dyn makes of those maps and of the tiled golden mask, next to zlib's inflate and a device copy, the same
entry next to fnn_inflate_segments on the fixed fragments, and the two folder commands over files written with
``compress_on_device='dynamic'``, read with ``inflate_on_device=True`` (the zlib fallback) and ``'dynamic'``; and
(``--section inflate_any``, these rows alone, written to profiles/r35_inflate_any.txt unless ``--out`` says otherwise)
fnn_inflate_stream on streams that zlib wrote against zlib's inflate on this machine and the folder commands on folders that
zlib wrote, read with ``inflate_on_device=True`` and ``'any'``.  ``--section read`` runs the file -> device rows of both files alone and
``--section predict_files`` the two predict_from_files rows alone, with the defaults of the full run: for repeating those
rows in many fresh processes (profiles/r24_host_prologue.txt).

The volume is synthetic: an int16 "CT" of n^3 voxels (smooth structure + noise, so that gzip has something to do), written
as .nii.gz (level 1, like the writer) and as .nii.

usage (repo root, GPU box): python tools/imageio_bench.py [--n 512] [--reps 3] [--cases 4] [--case-shape 96 192 192]
                                                          [--section all|reorient|deflate|masks|label_files|inflate|inflate_dyn|inflate_any|predict_files|read] [--out FILE]
"""
import argparse
import gzip
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_TBS = 6.29          # MI355X_MICROARCH: float4 copy, measured


def wall(fn, reps):
    ts, out = [], None
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), min(ts), max(ts), out


def events(fn, reps, dev):
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


def events_batched(fn, calls, windows, dev):
    """ms per call: `calls` calls of fn inside one pair of events, `windows` such windows after one warm-up window -> (median,
    min, max) of the windows' per-call times.  For calls of a fraction of a millisecond, whose single-call window would hold
    as much enqueue cost as kernel."""
    ts = []
    for r in range(windows + 1):
        torch.cuda.synchronize(dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        e1.synchronize()
        if r:
            ts.append(e0.elapsed_time(e1) / calls)
    return float(np.median(ts)), min(ts), max(ts)


def events_batched_pair(fa, fb, calls, windows, dev):
    """``events_batched`` for two calls that are compared: their windows alternate, so that both see the same machine ->
    the two (median, min, max)."""
    ts = ([], [])
    for r in range(windows + 1):                  # the first pair of windows is the warm-up
        for k, fn in enumerate((fa, fb)):
            torch.cuda.synchronize(dev)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                fn()
            e1.record()
            e1.synchronize()
            if r:
                ts[k].append(e0.elapsed_time(e1) / calls)
    return tuple((float(np.median(t)), min(t), max(t)) for t in ts)


def synthetic_ct(shape, seed):
    rng = np.random.default_rng(seed)
    z, y, x = np.meshgrid(*[np.linspace(-1, 1, s, dtype=np.float32) for s in shape], indexing='ij', sparse=True)
    body = (z * z * 0.8 + y * y + x * x) < 0.7
    v = np.where(body, 40 + 300 * np.sin(6 * x) * np.cos(5 * y + 3 * z), -1000).astype(np.float32)
    v += rng.integers(-12, 13, shape, dtype=np.int16)
    return v.astype(np.int16)


def bench_reorient(n, reps, dev, say, row):
    """fnn_reorient on n^3 elements: the decoded float32 voxels into the RAS frame (forward) and the uint8 labels back
    (backward), a flip-only orientation (the row path) and one that moves the fastest axis (the tiled transpose)."""
    from fast_nnunet_amd import capi
    from fast_nnunet_amd import imageio as fio
    stream = torch.cuda.current_stream(dev).cuda_stream
    say(f'--- fnn_reorient, {n}^3 elements; events around the call, the first call is the warm-up; numpy by wall clock')
    shape = (n, n, n)
    rng = np.random.default_rng(5)
    for what, dt, tdt in (('float32 forward', np.float32, torch.float32), ('uint8 backward', np.uint8, torch.uint8)):
        host = rng.integers(0, 200, shape, dtype=np.uint8).astype(dt)
        src = torch.from_numpy(host).to(dev)
        dst = torch.empty_like(src)
        moved = 2 * host.nbytes
        t = events(lambda: dst.copy_(src), reps, dev)
        row(f'{what}: device-to-device copy of the same bytes ({host.nbytes / 2 ** 20:.0f} MiB)', t, f'  {moved / t[0] / 1e6:.0f} GB/s')
        for path, src_axis, flip in (('flip only (rows)', (0, 1, 2), (0, 1, 1)), ('fastest axis moved (transpose)', (2, 0, 1), (0, 1, 0))):
            t = events(lambda: capi.reorient(src.data_ptr(), host.itemsize, shape, src_axis, flip, dst.data_ptr(), stream), reps, dev)
            row(f'{what}: fnn_reorient, {path}', t,
                f'  {moved / t[0] / 1e6:.0f} GB/s = {100 * moved / t[0] / 1e6 / (COPY_TBS * 1e3):.1f} % of {COPY_TBS} TB/s')
            same = np.array_equal(dst.cpu().numpy().reshape(-1)[::4099], fio.reorient_on_host(host, src_axis, flip).reshape(-1)[::4099])
            tn = wall(lambda: fio.reorient_on_host(host, src_axis, flip), reps)
            row(f'{what}: numpy flip / transpose on the host, {path}', tn[:3], f'  {tn[0] / t[0]:.0f}x the kernel; equal samples: {same}')
        del src, dst, host


def label_map(n, dev, seed=18, k=60):
    """A seeded map of n^3 voxels: k ellipsoids (labels 1 .. k, later ones on top) on background 0, made on the device."""
    g = torch.Generator().manual_seed(seed)
    centre, radius = torch.rand(k, 3, generator=g) * n, (0.04 + 0.14 * torch.rand(k, 3, generator=g)) * n
    ax = [torch.arange(n, dtype=torch.float32, device=dev).reshape([-1 if d == k else 1 for d in range(3)]) for k in range(3)]
    labels = torch.zeros((n, n, n), dtype=torch.uint8, device=dev)
    for k in range(k):
        inside = sum(((ax[d] - float(centre[k, d])) / float(radius[k, d])) ** 2 for d in range(3)) < 1.0
        labels[inside] = k + 1
    return labels


def bench_deflate(n, reps, dev, say, row):
    """fnn_deflate_labels (csrc/deflate.hip) against zlib level 1 on this machine's CPU and a device copy of the same bytes,
    and fnn_deflate_labels_dyn (csrc/deflate_dyn.hip) against both."""
    import zlib
    from fast_nnunet_amd import capi
    stream = torch.cuda.current_stream(dev).cuda_stream
    say(f'--- fnn_deflate_labels; events around the call (it allocates its scratch and synchronises), the first call is the '
        f'warm-up; zlib level 1 on this machine, one thread, by wall clock')
    golden = os.path.join(ROOT, 'tests', 'golden', 'example_ct_sm_T300_output.nii.gz')
    blob = gzip.decompress(open(golden, 'rb').read())
    mask = np.frombuffer(blob[352:], np.uint8).reshape(30, 101, 122)
    reps_of = [max(1, round(n / s)) for s in mask.shape]
    synth = label_map(n, dev)
    inputs = [(f'61 labels, uint8 {n}^3', synth), (f'61 labels, uint16 {n}^3 (values x 1000)', synth.to(torch.int16) * 1000),
              (f'golden mask tiled {reps_of} -> uint8 {tuple(r * s for r, s in zip(reps_of, mask.shape))}',
               torch.from_numpy(np.tile(mask, reps_of)).to(dev))]
    for name, labels in inputs:
        n_bytes = labels.numel() * labels.element_size()
        cap = capi.deflate_bound(n_bytes)
        out = torch.empty(cap, dtype=torch.uint8, device=dev)
        res = []
        t = events(lambda: res.append(capi.deflate_labels(labels.data_ptr(), labels.element_size(), labels.numel(), True,
                                                          out.data_ptr(), cap, stream)), reps, dev)
        n_out, file_size, crc = res[-1]
        say(f'{name}: {n_bytes / 2 ** 20:.0f} MiB of labels, {file_size} byte(s) per voxel in the file')
        row('  fnn_deflate_labels', t, f'  {n_bytes / t[0] / 1e6:.1f} GB/s of labels; fragment {n_out / 2 ** 20:.2f} MiB')
        dst = torch.empty_like(labels)
        tc = events(lambda: dst.copy_(labels), reps, dev)
        row('  device-to-device copy of the same bytes', tc, f'  {2 * n_bytes / tc[0] / 1e6:.0f} GB/s; the encoder takes {t[0] / tc[0]:.1f}x')
        del dst
        td = wall(lambda: labels.cpu(), reps)
        row(f'  download of the labels ({n_bytes / 2 ** 20:.0f} MiB, pageable)', td[:3], f'  {n_bytes / td[0] / 1e6:.1f} GB/s')
        tf = wall(lambda: out[:n_out].cpu(), reps)
        row(f'  download of the fragment ({n_out / 2 ** 20:.2f} MiB, pageable)', tf[:3])
        raw = td[3].numpy().tobytes()
        tz = wall(lambda: zlib.compress(raw, 1), 1)
        frag = tf[3].numpy().tobytes()
        d = zlib.decompressobj(-15)
        same = d.decompress(frag + b'\x03\x00') == raw and zlib.crc32(raw) == crc
        row('  zlib.compress(level 1) of the same bytes (host)', tz[:3],
            f'  {n_bytes / tz[0] / 1e6:.2f} GB/s; {len(tz[3]) / 2 ** 20:.2f} MiB: the fragment is {n_out / len(tz[3]):.2f}x that; '
            f'{tz[0] / t[0]:.0f}x the kernel\'s time')
        say(f'  the fragment inflates to the labels and the CRC is zlib\'s: {same}')
        # per-chunk dynamic Huffman tables (csrc/deflate_dyn.hip) next to the fixed call, the yardstick, in alternating windows
        out_d = torch.empty(cap, dtype=torch.uint8, device=dev)
        res_d = []
        tfix, tdyn = events_batched_pair(
            lambda: capi.deflate_labels(labels.data_ptr(), labels.element_size(), labels.numel(), True, out.data_ptr(), cap, stream),
            lambda: res_d.append(capi.deflate_labels_dyn(labels.data_ptr(), labels.element_size(), labels.numel(), True, out_d.data_ptr(), cap, stream)),
            10, 5, dev)
        n_dyn, _, crc_d, dynamic_chunks = res_d[-1]
        row('  fnn_deflate_labels, 10 calls per window, 5 windows', tfix, f'  fragment {n_out / 2 ** 20:.2f} MiB')
        row('  fnn_deflate_labels_dyn, the same windows in turn', tdyn,
            f'  {tdyn[0] / tfix[0]:.2f}x the fixed call; fragment {n_dyn / 2 ** 20:.2f} MiB = {n_dyn / n_out:.2f}x the fixed one; '
            f'{dynamic_chunks} of {-(-labels.numel() * file_size // 16384)} chunks took their own tables')
        tfd = wall(lambda: out_d[:n_dyn].cpu(), reps)
        row(f'  download of the dynamic fragment ({n_dyn / 2 ** 20:.2f} MiB, pageable)', tfd[:3], f'  the fixed one: {tf[0]:.2f} ms')
        frag_d = tfd[3].numpy().tobytes()
        d = zlib.decompressobj(-15)
        same = d.decompress(frag_d + b'\x03\x00') == raw and crc_d == crc
        tz6 = wall(lambda: zlib.compress(raw, 6), 1)
        say(f'  sizes: dynamic {n_dyn} B, fixed {n_out} B, zlib level 1 {len(tz[3])} B ({n_dyn / len(tz[3]):.2f}x), zlib level 6 '
            f'{len(tz6[3])} B ({n_dyn / len(tz6[3]):.2f}x; {tz6[0]:.0f} ms on the host)')
        say(f'  zlib level 1 on the host takes {tz[0] / tdyn[0]:.0f}x the dynamic call\'s time; the dynamic fragment inflates to the '
            f'labels and the CRC is zlib\'s: {same}')
        del out, out_d, raw, frag, frag_d, labels
    del inputs, synth


def bench_masks(n, reps, dev, say, row):
    """fnn_deflate_masks_count + fnn_deflate_masks_emit (csrc/deflate_masks.hip): every foreground label's mask of one map."""
    import zlib
    from fast_nnunet_amd import capi
    stream = torch.cuda.current_stream(dev).cuda_stream
    C = 16384
    say('--- fnn_deflate_masks_count + fnn_deflate_masks_emit: one uint8 mask fragment per foreground label; events around the '
        'calls (work and out allocated before), the first call is the warm-up; zlib level 1 on this machine, one thread, by wall clock')
    golden = os.path.join(ROOT, 'tests', 'golden', 'example_ct_sm_T300_output.nii.gz')
    mask = np.frombuffer(gzip.decompress(open(golden, 'rb').read())[352:], np.uint8).reshape(30, 101, 122)
    reps_of = [max(1, round(n / s)) for s in mask.shape]
    synth61, synth118 = label_map(n, dev), label_map(n, dev, k=117)
    inputs = [(f'61 labels (60 masks), uint8 {n}^3', synth61, list(range(1, 61))),
              (f'118 labels (117 masks), uint8 {n}^3', synth118, list(range(1, 118))),
              (f'118 labels (117 masks), 2-byte {n}^3 (values x 257)', synth118.to(torch.int16) * 257, [257 * i for i in range(1, 118)]),
              (f'golden mask tiled {reps_of} -> uint8 {tuple(r * s for r, s in zip(reps_of, mask.shape))}',
               torch.from_numpy(np.tile(mask, reps_of)).to(dev), [int(i) for i in np.unique(mask) if i])]
    del synth61, synth118
    for name, labels, wanted in inputs:
        labels = labels.contiguous()
        nel, size, L = labels.numel(), labels.element_size(), len(wanted)
        chunks = (nel + C - 1) // C
        flat = labels.reshape(-1).to(torch.int64) & 0xFFFF
        pad = torch.nn.functional.pad(flat, (0, chunks * C - nel), value=int(flat[-1])).view(chunks, C)
        seen = torch.zeros((chunks, 65536 if size == 2 else 256), dtype=torch.uint8, device=dev)
        seen.scatter_(1, pad, 1)
        pairs = int(seen[:, wanted].sum()) + (L - int(seen[-1, wanted].sum()) if nel % C else 0)
        del flat, pad, seen
        work_cap = capi.deflate_masks_work_bytes(nel, L)
        work = torch.empty(work_cap, dtype=torch.uint8, device=dev)
        res = []
        t_count = events(lambda: res.append(capi.deflate_masks_count(labels.data_ptr(), size, nel, wanted, work.data_ptr(), work_cap, stream)),
                         reps, dev)
        sizes, crcs = res[-1]
        total = sum(sizes)
        out = torch.empty(total, dtype=torch.uint8, device=dev)
        t_emit = events(lambda: capi.deflate_masks_emit(labels.data_ptr(), size, nel, wanted, work.data_ptr(), out.data_ptr(), total, stream),
                        reps, dev)

        def both():
            capi.deflate_masks_count(labels.data_ptr(), size, nel, wanted, work.data_ptr(), work_cap, stream)
            capi.deflate_masks_emit(labels.data_ptr(), size, nel, wanted, work.data_ptr(), out.data_ptr(), total, stream)
        t = events(both, reps, dev)
        say(f'{name}: {nel * size / 2 ** 20:.0f} MiB of labels, {L} masks of {nel / 2 ** 20:.0f} MiB; {chunks} chunks, '
            f'{pairs} of {chunks * L} (chunk, label) pairs are walked = {pairs / chunks:.2f} walks of the volume; work {work_cap / 2 ** 20:.1f} MiB')
        row('  count + emit', t, f'  {L * nel / t[0] / 1e6:.0f} GB/s of mask bytes; all fragments {total / 2 ** 20:.2f} MiB')
        row('    fnn_deflate_masks_count alone (synchronises)', t_count)
        row('    fnn_deflate_masks_emit alone', t_emit)
        # (a) what there was before: every mask materialised on the device and encoded by fnn_deflate_labels
        cap = capi.deflate_bound(nel)
        out_a = torch.empty(cap, dtype=torch.uint8, device=dev)
        got_a = []

        def one_by_one():
            got_a.clear()
            for v in wanted:
                m = (labels == v).to(torch.uint8)
                got_a.append(capi.deflate_labels(m.data_ptr(), 1, nel, False, out_a.data_ptr(), cap, stream)[0])
        ta = events(one_by_one, reps, dev)
        row(f'  (a) {L} x (mask on the device + fnn_deflate_labels)', ta,
            f'  {ta[0] / t[0]:.1f}x count + emit; fragments {sum(got_a) / 2 ** 20:.2f} MiB, here {total / sum(got_a):.2f}x that')
        # (b) the host writer: zlib level 1 of one mask, times the number of masks
        mid = L // 2
        host_mask = (labels == wanted[mid]).to(torch.uint8).cpu().numpy().tobytes()
        tz = wall(lambda: zlib.compress(host_mask, 1), 1)
        empty = zlib.compress(bytes(nel), 1)
        row(f'  (b) zlib.compress(level 1) of one mask (host), label {wanted[mid]}', tz[:3],
            f'  x {L} masks = {tz[0] * L / 1e3:.1f} s = {tz[0] * L / t[0]:.0f}x count + emit; {len(tz[3])} B, its fragment {sizes[mid]} B '
            f'= {sizes[mid] / len(tz[3]):.2f}x; an empty mask: zlib {len(empty)} B, fragment {112 * (nel // C)} B + the last chunk')
        # (c) what is downloaded
        td = wall(lambda: out.cpu(), reps)
        row(f'  (c) download of all fragments ({total / 2 ** 20:.2f} MiB, pageable)', td[:3],
            f'  the label map is {nel * size / 2 ** 20:.0f} MiB, the masks {L * nel / 2 ** 20:.0f} MiB')
        blob = td[3].numpy()
        at = sum(sizes[:mid])
        d = zlib.decompressobj(-15)
        same = d.decompress(blob[at:at + sizes[mid]].tobytes() + b'\x03\x00') == host_mask and zlib.crc32(host_mask) == crcs[mid]
        say(f'  the fragment of label {wanted[mid]} inflates to its mask and the CRC is zlib\'s: {same}')
        del out, out_a, work, labels, blob, host_mask
    del inputs


def bench_label_files(n, reps, cases, dev, say, row):
    """fnn_decode_labels (csrc/imageio.hip) and the folder evaluation that reads with it."""
    from fast_nnunet_amd import capi
    from fast_nnunet_amd import evaluation as ev
    from fast_nnunet_amd import imageio as fio
    stream = torch.cuda.current_stream(dev).cuda_stream
    calls, windows = 100, max(reps, 5)
    say(f'--- fnn_decode_labels, a 61-label map of {n}^3 voxels; outputs allocated before; ms per call from {calls} calls inside one '
        f'pair of events, median (min, max) of {windows} such windows after a warm-up window')
    labels = label_map(n, dev)
    n_vox = labels.numel()
    status = torch.zeros(2, dtype=torch.int32, device=dev)
    f32 = torch.empty(n_vox, dtype=torch.float32, device=dev)
    for what, code, size, raw, out_dt in (('int16 file bytes -> 2-byte labels', 4, 2, labels.to(torch.int16).reshape(-1).view(torch.uint8), torch.int16),
                                          ('uint8 file bytes -> uint8 labels', 2, 1, labels.reshape(-1), torch.uint8)):
        raw = raw.contiguous()
        out = torch.empty(n_vox, dtype=out_dt, device=dev)
        moved = n_vox * size * 2
        t = events_batched(lambda: capi.decode_labels(raw.data_ptr(), code, False, n_vox, False, 1.0, 0.0, size, out.data_ptr(),
                                                      status.data_ptr(), stream), calls, windows, dev)
        row(f'{what}: fnn_decode_labels', t,
            f'  {moved / t[0] / 1e6:.0f} GB/s of {moved / 1e9:.2f} GB = {100 * moved / t[0] / 1e6 / (COPY_TBS * 1e3):.1f} % of {COPY_TBS} TB/s; '
            f'status {status.tolist()}')
        same = bool((out.reshape(labels.shape) == labels).all())

        def before():
            capi.decode_voxels(raw.data_ptr(), code, False, n_vox, False, 1.0, 0.0, f32.data_ptr(), stream)
            out.copy_(f32)
        tb = events_batched(before, calls, windows, dev)
        row(f'{what}: fnn_decode_voxels + the cast of its float32 ({4 * n_vox / 2 ** 20:.0f} MiB)', tb, f'  {tb[0] / t[0]:.1f}x fnn_decode_labels')
        dst = torch.empty_like(raw)
        tc = events_batched(lambda: dst.copy_(raw), calls, windows, dev)
        row(f'{what}: device copy of the same bytes ({n_vox * size / 2 ** 20:.0f} MiB)', tc,
            f'  {moved / tc[0] / 1e6:.0f} GB/s; the decode takes {t[0] / tc[0]:.2f}x; labels equal the map: {same}')
        del out, dst, raw
    del f32

    say(f'--- compute_metrics_on_folder, {cases} cases of {n}^3 voxels: uint8 .nii.gz references, int16 .nii.gz predictions (gzip level 1), '
        f'60 foreground labels; wall clock')
    with tempfile.TemporaryDirectory() as tmp:
        ref_dir, pred_dir = os.path.join(tmp, 'ref'), os.path.join(tmp, 'pred')
        os.makedirs(ref_dir), os.makedirs(pred_dir)
        affine = np.diag([0.8, 0.8, 1.25, 1.0])
        for i in range(cases):
            ref = label_map(n, dev, seed=30 + i)
            pred = ref.clone()
            pred[i::7] = 0
            for folder, arr, code in ((ref_dir, ref.cpu().numpy(), 2), (pred_dir, pred.cpu().numpy().astype('<i2'), 4)):
                with open(os.path.join(folder, f'case{i}.nii.gz'), 'wb') as raw, \
                        gzip.GzipFile(filename='', mode='wb', compresslevel=1, fileobj=raw, mtime=0) as g:
                    g.write(fio.nifti1_header_bytes((n, n, n), code, affine))
                    g.write(arr.tobytes())
            del ref, pred
        sizes = [os.path.getsize(os.path.join(d, 'case0.nii.gz')) / 2 ** 20 for d in (ref_dir, pred_dir)]
        say(f'case0 on disk: reference {sizes[0]:.1f} MiB, prediction {sizes[1]:.1f} MiB')
        rw = fio.NiftiIO(dev)
        lor = list(range(1, 61))
        ev.compute_metrics_on_folder(ref_dir, pred_dir, None, rw, '.nii.gz', lor)                    # warm-up
        t = wall(lambda: ev.compute_metrics_on_folder(ref_dir, pred_dir, os.path.join(pred_dir, 'summary.json'), rw, '.nii.gz', lor), reps)
        row(f'compute_metrics_on_folder, {cases} cases (reader thread)', t[:3], f'  {t[0] / cases:.1f} ms per case')
        pair = [os.path.join(ref_dir, 'case0.nii.gz'), os.path.join(pred_dir, 'case0.nii.gz')]
        staged = rw.stage_label_files(pair)
        row('  one case, inflate: both files into pinned memory (host)', wall(staged.fill, reps)[:3])
        raws = [torch.empty(h.n_bytes, dtype=torch.uint8, device=dev) for h in staged.hdrs]
        outs = [torch.empty(h.shape, dtype=torch.uint8 if h.bytes_per_voxel == 1 else torch.int16, device=dev) for h in staged.hdrs]
        total = sum(h.n_bytes for h in staged.hdrs)
        tu = events(lambda: [r.copy_(b[:h.n_bytes], non_blocking=True) for r, b, h in zip(raws, staged.buffers, staged.hdrs)], reps, dev)
        row(f'  one case, upload: both files ({total / 2 ** 20:.0f} MiB, pinned)', tu, f'  {total / tu[0] / 1e6:.1f} GB/s')
        td = events(lambda: [capi.decode_labels(r.data_ptr(), h.datatype, h.byteswap, h.n_vox, h.scale, h.slope, h.inter,
                                                fio.label_bytes(h), o.data_ptr(), status.data_ptr(), stream)
                             for r, o, h in zip(raws, outs, staged.hdrs)], reps, dev)
        row('  one case, decode: fnn_decode_labels on both', td)
        values = ev.count_classes(lor)
        tcnt = wall(lambda: ev.confusion_counts(outs[0], [outs[1]], values, None, checked=True), reps)
        row('  one case, count: confusion_counts (uint8 against 2-byte: the reference map is widened first)', tcnt[:3])
        narrow = outs[1].to(torch.uint8)
        tcn = wall(lambda: ev.confusion_counts(outs[0], [narrow], values, None, checked=True), reps)
        row('  one case, count: confusion_counts after the narrowing read_label_map does (uint8 against uint8)', tcn[:3])
        row('  one case, decode_label_maps (upload, decode, status, narrowing)', wall(lambda: rw.decode_label_maps(staged), reps)[:3])


def bench_inflate(n, reps, cases, dev, say, row):
    """fnn_inflate_segments (csrc/inflate.hip) against zlib's inflate on this machine's CPU and a device copy of the output,
    and the folder commands that read with it."""
    import zlib
    from fast_nnunet_amd import capi
    from fast_nnunet_amd import evaluation as ev
    from fast_nnunet_amd import imageio as fio
    from fast_nnunet_amd import postprocessing as pp
    stream = torch.cuda.current_stream(dev).cuda_stream
    calls, windows = 10, max(reps, 5)
    say(f'--- fnn_inflate_segments on fragments made by the device encoders; in and out allocated before, the call allocates its '
        f'scratch and synchronises; ms per call from {calls} calls inside one pair of events, median (min, max) of {windows} such '
        f'windows after a warm-up window; zlib on this machine, one thread, by wall clock')

    def candidates(frag):
        return np.array([0] + [e for e in fio._marker_ends(frag, 0, len(frag)) if e < len(frag)], dtype=np.int64)

    synth = label_map(n, dev)
    noise = torch.randint(0, 61, (n, n, n), dtype=torch.uint8, device=dev, generator=torch.Generator(dev).manual_seed(7))
    inputs = [(f'61 labels, uint8 {n}^3 (long runs)', synth), (f'61 labels, uint16 {n}^3 (values x 1000; long runs)', synth.to(torch.int16) * 1000),
              (f'random labels 0 .. 60, uint8 {n}^3 (no runs: every byte a literal)', noise)]
    for name, labels in inputs:
        n_bytes = labels.numel() * labels.element_size()
        cap = capi.deflate_bound(n_bytes)
        frag_dev = torch.empty(cap, dtype=torch.uint8, device=dev)
        n_in, _, crc_enc = capi.deflate_labels(labels.data_ptr(), labels.element_size(), labels.numel(), False, frag_dev.data_ptr(), cap, stream)
        frag = frag_dev[:n_in].cpu().numpy().tobytes()
        tscan = wall(lambda: candidates(frag), reps)
        starts = tscan[3]
        out = torch.empty(n_bytes, dtype=torch.uint8, device=dev)
        res = []
        t = events_batched(lambda: res.append(capi.inflate_segments(frag_dev.data_ptr(), n_in, starts, out.data_ptr(), n_bytes, stream)),
                           calls, windows, dev)
        same = res[-1] == (0, crc_enc) and bool((out == labels.reshape(-1).view(torch.uint8)).all())
        say(f'{name}: fragment {n_in / 2 ** 20:.2f} MiB -> {n_bytes / 2 ** 20:.0f} MiB, {len(starts)} candidates')
        row('  fnn_inflate_segments (count pass, chain on the host, emit pass)', t,
            f'  {n_bytes / t[0] / 1e6:.1f} GB/s of output; status and CRC good, bytes equal the map: {same}')
        row('  host: candidate scan of the fragment (bytes.find)', tscan[:3])
        dst = torch.empty_like(out)
        tc = events_batched(lambda: dst.copy_(out), calls, windows, dev)
        fits = '; a cache rate: source and destination fit the Infinity Cache' if 2 * n_bytes <= 256 * 2 ** 20 else ''
        row('  device-to-device copy of the output bytes', tc, f'  {2 * n_bytes / tc[0] / 1e6:.0f} GB/s; the decoder takes {t[0] / tc[0]:.0f}x{fits}')
        tz = wall(lambda: zlib.decompressobj(-15).decompress(frag + b'\x03\x00'), reps)
        row('  zlib inflate of the same fragment (host)', tz[:3],
            f'  {n_bytes / tz[0] / 1e6:.2f} GB/s; {tz[0] / t[0]:.0f}x the device call\'s time; CRC equal: {zlib.crc32(tz[3]) == res[-1][1]}')
        host_file = zlib.compress(tz[3], 1)
        tzz = wall(lambda: zlib.decompress(host_file), reps)
        row(f'  zlib inflate of zlib\'s own level-1 stream of these bytes ({len(host_file) / 2 ** 20:.2f} MiB, host)', tzz[:3])
        del frag_dev, out, dst, frag, host_file
    del noise, inputs

    wanted = list(range(1, 61))
    nel = synth.numel()
    work_cap = capi.deflate_masks_work_bytes(nel, len(wanted))
    work = torch.empty(work_cap, dtype=torch.uint8, device=dev)
    sizes, crcs = capi.deflate_masks_count(synth.data_ptr(), 1, nel, wanted, work.data_ptr(), work_cap, stream)
    blob_dev = torch.empty(sum(sizes), dtype=torch.uint8, device=dev)
    capi.deflate_masks_emit(synth.data_ptr(), 1, nel, wanted, work.data_ptr(), blob_dev.data_ptr(), sum(sizes), stream)
    blob = blob_dev.cpu().numpy().tobytes()
    frags, at = [], 0
    for nb in sizes:
        frags.append(blob[at:at + nb])
        at += nb
    frag_devs = [torch.frombuffer(bytearray(f), dtype=torch.uint8).to(dev) for f in frags]      # each 16-byte aligned
    startss = [candidates(f) for f in frags]
    out = torch.empty(nel, dtype=torch.uint8, device=dev)
    got = []

    def all_masks():
        got.clear()
        for fd, f, st in zip(frag_devs, frags, startss):
            got.append(capi.inflate_segments(fd.data_ptr(), len(f), st, out.data_ptr(), nel, stream))
    t = events_batched(all_masks, 1, windows, dev)
    good = got == [(0, c) for c in crcs] and bool((out == (synth.reshape(-1) == wanted[-1])).all())
    say(f'60 masks of the 61-label map: fragments {sum(sizes) / 2 ** 20:.2f} MiB -> 60 x {nel / 2 ** 20:.0f} MiB, {sum(len(s) for s in startss)} candidates')
    row('  60 x fnn_inflate_segments, one per mask, into one buffer', t,
        f'  {t[0] / 60:.2f} ms per mask, {60 * nel / t[0] / 1e6:.0f} GB/s of mask bytes; status and CRCs good, the last mask equal: {good}')
    mid = 30
    tz = wall(lambda: zlib.decompressobj(-15).decompress(frags[mid] + b'\x03\x00'), reps)
    row(f'  zlib inflate of one mask\'s fragment (host), label {wanted[mid]}', tz[:3], f'  x 60 = {60 * tz[0]:.0f} ms = {60 * tz[0] / t[0]:.0f}x')
    del work, blob_dev, frag_devs, out, frags, blob

    say(f'--- folder commands, {cases} cases of {n}^3 voxels, 60 foreground labels: predictions written with compress_on_device=True; '
        f'per-case wall clock with inflate_on_device off (the route before) and on')
    plans = {'dataset_name': 'd', 'plans_name': 'p', 'image_reader_writer': 'NibabelIO', 'configurations': {}}
    dj = {'labels': dict({'background': 0}, **{f'l{i}': i for i in wanted}), 'file_ending': '.nii.gz', 'channel_names': {'0': 'CT'}}
    with tempfile.TemporaryDirectory() as tmp:
        ref_z, ref_d, pred_dir = (os.path.join(tmp, d) for d in ('ref_zlib', 'ref_device', 'pred'))
        for d in (ref_z, ref_d, pred_dir):
            os.makedirs(d)
        writer = fio.NiftiIO(dev)
        props = {'nibabel_stuff': {'original_affine': np.diag([0.8, 0.8, 1.25, 1.0])}}
        for i in range(cases):
            ref = label_map(n, dev, seed=30 + i)
            pred = ref.clone()
            pred[i::7] = 0
            writer.write_seg(ref.cpu().numpy(), os.path.join(ref_z, f'case{i}.nii.gz'), props)
            writer.write_seg(writer.compress_labels(ref, props), os.path.join(ref_d, f'case{i}.nii.gz'), props)
            writer.write_seg(writer.compress_labels(pred, props), os.path.join(pred_dir, f'case{i}.nii.gz'), props)
            del ref, pred
        sizes = [os.path.getsize(os.path.join(d, 'case0.nii.gz')) / 2 ** 20 for d in (ref_z, ref_d, pred_dir)]
        say(f'case0 on disk: reference by zlib {sizes[0]:.1f} MiB, reference by the device {sizes[1]:.1f} MiB, prediction {sizes[2]:.1f} MiB')
        for what, ref_dir in (('references written by zlib (they inflate on the host either way)', ref_z), ('references written on the device too', ref_d)):
            made = {}
            for flag in (False, True):
                rw = fio.NiftiIO(dev, inflate_on_device=flag)
                ev.compute_metrics_on_folder(ref_dir, pred_dir, None, rw, '.nii.gz', wanted)                 # warm-up
                t = wall(lambda: ev.compute_metrics_on_folder(ref_dir, pred_dir, None, rw, '.nii.gz', wanted), reps)
                made[flag] = t
                row(f'compute_metrics_on_folder, {what[:34]}.., flag {"on" if flag else "off"}', t[:3],
                    f'  {t[0] / cases:.1f} ms per case; routes {rw.inflate_stats}')
            say(f'  {what}: {made[False][0] / made[True][0]:.2f}x; equal results: {repr(made[False][3]) == repr(made[True][3])}')
        fns, kwargs = [pp.remove_all_but_largest_component_from_segmentation], [{'labels_or_regions': wanted}]
        made = {}
        for flag in (False, True):
            out_dir = os.path.join(tmp, f'post_{int(flag)}')
            run = lambda: pp.apply_postprocessing_to_folder(pred_dir, out_dir, fns, kwargs, plans, dj, compress_on_device=True,   # noqa: E731
                                                            inflate_on_device=flag)
            run()                                                                                            # warm-up
            made[flag] = wall(run, reps)
            row(f'apply_postprocessing_to_folder (compress_on_device), flag {"on" if flag else "off"}', made[flag][:3],
                f'  {made[flag][0] / cases:.1f} ms per case')
        same = all(open(os.path.join(tmp, 'post_0', f'case{i}.nii.gz'), 'rb').read() == open(os.path.join(tmp, 'post_1', f'case{i}.nii.gz'), 'rb').read()
                   for i in range(cases))
        say(f'  apply_postprocessing_to_folder: {made[False][0] / made[True][0]:.2f}x; identical output files: {same}')
        pair = [os.path.join(ref_d, 'case0.nii.gz'), os.path.join(pred_dir, 'case0.nii.gz')]
        for flag in (False, True):
            rw = fio.NiftiIO(dev, inflate_on_device=flag)
            staged = rw.stage_label_files(pair)
            row(f'  one case, both files device-written, flag {"on" if flag else "off"}: StagedCase.fill (host)', wall(staged.fill, reps)[:3])
            row(f'  one case, both files device-written, flag {"on" if flag else "off"}: decode_label_maps', wall(lambda: rw.decode_label_maps(staged), reps)[:3])


def bench_inflate_dyn(n, reps, cases, dev, say, row):
    """fnn_inflate_segments_dyn (csrc/inflate_dyn.hip) on the fragments of fnn_deflate_labels_dyn against zlib's inflate on this
    machine's CPU and a device copy of the output; the same entry on the fixed fragment next to fnn_inflate_segments (what
    the general kernels cost a fixed-only file); and the folder commands on files written with compress_on_device='dynamic',
    read with inflate_on_device=True (the zlib fallback) and 'dynamic'."""
    import zlib
    from fast_nnunet_amd import capi
    from fast_nnunet_amd import evaluation as ev
    from fast_nnunet_amd import imageio as fio
    from fast_nnunet_amd import postprocessing as pp
    stream = torch.cuda.current_stream(dev).cuda_stream
    calls, windows = 10, max(reps, 5)
    say(f'--- fnn_inflate_segments_dyn on fragments made by fnn_deflate_labels_dyn (dynamic) and fnn_deflate_labels (fixed); in and '
        f'out allocated before, the call allocates its scratch and synchronises; ms per call from {calls} calls inside one pair of '
        f'events, median (min, max) of {windows} such windows after a warm-up window, the windows of two calls that are compared '
        f'in turn; zlib on this machine, one thread, by wall clock')

    def candidates(frag):
        return np.array([0] + [e for e in fio._marker_ends(frag, 0, len(frag)) if e < len(frag)], dtype=np.int64)

    golden = os.path.join(ROOT, 'tests', 'golden', 'example_ct_sm_T300_output.nii.gz')
    mask = np.frombuffer(gzip.decompress(open(golden, 'rb').read())[352:], np.uint8).reshape(30, 101, 122)
    reps_of = [max(1, round(n / s)) for s in mask.shape]
    synth = label_map(n, dev)
    noise = torch.randint(0, 61, (n, n, n), dtype=torch.uint8, device=dev, generator=torch.Generator(dev).manual_seed(7))
    inputs = [(f'61 labels, uint8 {n}^3 (long runs)', synth), (f'61 labels, uint16 {n}^3 (values x 1000; long runs)', synth.to(torch.int16) * 1000),
              (f'golden mask tiled {reps_of} -> uint8 {tuple(r * s for r, s in zip(reps_of, mask.shape))}', torch.from_numpy(np.tile(mask, reps_of)).to(dev)),
              (f'random labels 0 .. 60, uint8 {n}^3 (no runs: every byte a literal)', noise)]
    for name, labels in inputs:
        n_bytes = labels.numel() * labels.element_size()
        cap = capi.deflate_bound(n_bytes)
        made = {}
        for kind in ('dynamic', 'fixed'):
            buf = torch.empty(cap, dtype=torch.uint8, device=dev)
            if kind == 'dynamic':
                n_in, _, crc_enc, dynamic_chunks = capi.deflate_labels_dyn(labels.data_ptr(), labels.element_size(), labels.numel(), False, buf.data_ptr(), cap, stream)
            else:
                n_in, _, crc_enc = capi.deflate_labels(labels.data_ptr(), labels.element_size(), labels.numel(), False, buf.data_ptr(), cap, stream)
            frag = buf[:n_in].cpu().numpy().tobytes()
            made[kind] = (buf, n_in, crc_enc, frag, candidates(frag))
        out = torch.empty(n_bytes, dtype=torch.uint8, device=dev)
        want = labels.reshape(-1).view(torch.uint8)
        say(f'{name}: {n_bytes / 2 ** 20:.0f} MiB; dynamic fragment {made["dynamic"][1] / 2 ** 20:.2f} MiB ({dynamic_chunks} of '
            f'{-(-n_bytes // 16384)} chunks with their own tables, {len(made["dynamic"][4])} candidates), fixed fragment '
            f'{made["fixed"][1] / 2 ** 20:.2f} MiB ({len(made["fixed"][4])} candidates)')
        buf, n_in, crc_enc, frag, starts = made['dynamic']
        res = []
        t = events_batched(lambda: res.append(capi.inflate_segments_dyn(buf.data_ptr(), n_in, starts, out.data_ptr(), n_bytes, stream)), calls, windows, dev)
        same = res[-1] == (0, crc_enc) and bool((out == want).all())
        row('  fnn_inflate_segments_dyn on the dynamic fragment', t,
            f'  {n_bytes / t[0] / 1e6:.1f} GB/s of output; status and CRC good, bytes equal the map: {same}')
        refused = capi.inflate_segments(buf.data_ptr(), n_in, starts, out.data_ptr(), n_bytes, stream)
        say(f'  fnn_inflate_segments on the dynamic fragment: status {capi.INFLATE_REASONS[refused[0]]}')
        tz = wall(lambda: zlib.decompressobj(-15).decompress(frag + b'\x03\x00'), reps)
        row('  zlib inflate of the dynamic fragment (host)', tz[:3],
            f'  {n_bytes / tz[0] / 1e6:.2f} GB/s; {tz[0] / t[0]:.1f}x the device call\'s time; CRC equal: {zlib.crc32(tz[3]) == res[-1][1]}')
        dst = torch.empty_like(out)
        tc = events_batched(lambda: dst.copy_(out), calls, windows, dev)
        row('  device-to-device copy of the output bytes', tc, f'  {2 * n_bytes / tc[0] / 1e6:.0f} GB/s; the decoder takes {t[0] / tc[0]:.0f}x')
        buf_f, n_f, crc_f, frag_f, starts_f = made['fixed']
        res_a, res_b = [], []
        tfix, tgen = events_batched_pair(
            lambda: res_a.append(capi.inflate_segments(buf_f.data_ptr(), n_f, starts_f, out.data_ptr(), n_bytes, stream)),
            lambda: res_b.append(capi.inflate_segments_dyn(buf_f.data_ptr(), n_f, starts_f, out.data_ptr(), n_bytes, stream)), calls, windows, dev)
        row('  fnn_inflate_segments on the fixed fragment', tfix, f'  {n_bytes / tfix[0] / 1e6:.1f} GB/s of output')
        row('  fnn_inflate_segments_dyn on the fixed fragment, windows in turn', tgen,
            f'  {tgen[0] / tfix[0]:.2f}x the fixed entry; equal status and CRC: {res_a[-1] == res_b[-1] == (0, crc_f)}; the dynamic fragment '
            f'takes {t[0] / tfix[0]:.2f}x the fixed route on the fixed fragment')
        tzf = wall(lambda: zlib.decompressobj(-15).decompress(frag_f + b'\x03\x00'), reps)
        row('  zlib inflate of the fixed fragment (host)', tzf[:3])
        del made, buf, buf_f, out, dst, frag, frag_f, labels
    del noise, inputs

    wanted = list(range(1, 61))
    say(f'--- folder commands, {cases} cases of {n}^3 voxels, 60 foreground labels: every file written with compress_on_device=\'dynamic\'; '
        f'per-case wall clock with inflate_on_device=True (every file falls back to zlib) and \'dynamic\'')
    plans = {'dataset_name': 'd', 'plans_name': 'p', 'image_reader_writer': 'NibabelIO', 'configurations': {}}
    dj = {'labels': dict({'background': 0}, **{f'l{i}': i for i in wanted}), 'file_ending': '.nii.gz', 'channel_names': {'0': 'CT'}}
    with tempfile.TemporaryDirectory() as tmp:
        ref_d, pred_dir = (os.path.join(tmp, d) for d in ('ref_device', 'pred'))
        for d in (ref_d, pred_dir):
            os.makedirs(d)
        writer = fio.NiftiIO(dev)
        props = {'nibabel_stuff': {'original_affine': np.diag([0.8, 0.8, 1.25, 1.0])}}
        for i in range(cases):
            ref = label_map(n, dev, seed=30 + i)
            pred = ref.clone()
            pred[i::7] = 0
            writer.write_seg(writer.compress_labels(ref, props, tables='dynamic'), os.path.join(ref_d, f'case{i}.nii.gz'), props)
            writer.write_seg(writer.compress_labels(pred, props, tables='dynamic'), os.path.join(pred_dir, f'case{i}.nii.gz'), props)
            del ref, pred
        say(f'case0 on disk: reference {os.path.getsize(os.path.join(ref_d, "case0.nii.gz")) / 2 ** 20:.1f} MiB, prediction '
            f'{os.path.getsize(os.path.join(pred_dir, "case0.nii.gz")) / 2 ** 20:.1f} MiB')
        made = {}
        for flag in (True, 'dynamic'):
            rw = fio.NiftiIO(dev, inflate_on_device=flag)
            ev.compute_metrics_on_folder(ref_d, pred_dir, None, rw, '.nii.gz', wanted)                       # warm-up
            made[flag] = wall(lambda: ev.compute_metrics_on_folder(ref_d, pred_dir, None, rw, '.nii.gz', wanted), reps)
            row(f'compute_metrics_on_folder, inflate_on_device={flag!r}', made[flag][:3], f'  {made[flag][0] / cases:.1f} ms per case; routes {rw.inflate_stats}')
        say(f'  compute_metrics_on_folder: {made[True][0] / made["dynamic"][0]:.2f}x; equal results: {repr(made[True][3]) == repr(made["dynamic"][3])}')
        fns, kwargs = [pp.remove_all_but_largest_component_from_segmentation], [{'labels_or_regions': wanted}]
        made = {}
        for flag in (True, 'dynamic'):
            out_dir = os.path.join(tmp, f'post_{flag}')
            run = lambda: pp.apply_postprocessing_to_folder(pred_dir, out_dir, fns, kwargs, plans, dj, compress_on_device='dynamic',   # noqa: E731
                                                            inflate_on_device=flag)
            run()                                                                                            # warm-up
            made[flag] = wall(run, reps)
            row(f'apply_postprocessing_to_folder (dynamic files out), inflate_on_device={flag!r}', made[flag][:3], f'  {made[flag][0] / cases:.1f} ms per case')
        same = all(open(os.path.join(tmp, 'post_True', f'case{i}.nii.gz'), 'rb').read() == open(os.path.join(tmp, 'post_dynamic', f'case{i}.nii.gz'), 'rb').read()
                   for i in range(cases))
        say(f'  apply_postprocessing_to_folder: {made[True][0] / made["dynamic"][0]:.2f}x; identical output files: {same}')
    say('--- decoder: the kernels decode canonically across lanes (ballot of 15 limits, one LDS read per symbol; 75 ballots '
        'build a block\'s literal / length code).  The two-level lookup table was not built, so no row compares the two: the '
        'cost of the general decoder is the "fixed fragment" pair of rows above, and what a table decoder would change is open.')


def bench_inflate_any(n, reps, cases, dev, say, row):
    """fnn_inflate_stream (csrc/inflate_any.hip) on streams that zlib wrote - label maps at levels 1 and 6 as uint8 and uint16,
    their level-0 and Z_FIXED streams (one member: the worst cases) and a synthetic int16 CT volume at level 6 - against zlib's
    inflate of the same stream on this machine's CPU in the same run and fnn_inflate_segments_dyn on the project's own
    dynamic fragment of the same map; the block finder alone (fnn_inflate_find_blocks); and the folder commands on folders
    that zlib wrote, read with inflate_on_device=True (the parent's behaviour: every file on the host) and 'any'.  The times
    of the single kernels and the number of members (the emit kernel's grid) come from a kernel trace of this section."""
    import zlib
    from fast_nnunet_amd import capi
    from fast_nnunet_amd import evaluation as ev
    from fast_nnunet_amd import imageio as fio
    from fast_nnunet_amd import postprocessing as pp
    stream = torch.cuda.current_stream(dev).cuda_stream
    calls, windows = 10, max(reps, 5)
    say(f'--- fnn_inflate_stream on raw deflate streams made by zlib on this machine; in and out allocated before, the call allocates '
        f'its scratch and synchronises; ms per call from {calls} calls inside one pair of events (1 call for the one-member streams), '
        f'median (min, max) of {windows} such windows after a warm-up window; zlib on this machine, one thread, by wall clock')
    golden = os.path.join(ROOT, 'tests', 'golden', 'example_ct_sm_T300_output.nii.gz')
    mask = np.frombuffer(gzip.decompress(open(golden, 'rb').read())[352:], np.uint8).reshape(30, 101, 122)
    reps_of = [max(1, round(n / s)) for s in mask.shape]
    synth = label_map(n, dev)
    tiled = torch.from_numpy(np.tile(mask, reps_of)).to(dev)
    maps = [(f'61 labels {n}^3', synth), (f'golden mask tiled to {tuple(tiled.shape)}', tiled)]
    inputs = []
    for name, m in maps:
        for wide in (False, True):
            labels = m.to(torch.int16) * 1000 if wide else m
            for what, level, strategy in (('level 1', 1, zlib.Z_DEFAULT_STRATEGY), ('level 6', 6, zlib.Z_DEFAULT_STRATEGY)) + \
                    (() if wide else (('level 0 (stored: one member)', 0, zlib.Z_DEFAULT_STRATEGY), ('level 6 Z_FIXED (one member)', 6, zlib.Z_FIXED))):
                inputs.append((f'{name}, {"uint16 (values x 1000)" if wide else "uint8"}, {what}', labels, level, strategy, (name, wide)))
    ct = torch.from_numpy(synthetic_ct((n, n, n), 1)).to(dev)
    inputs.append((f'synthetic CT int16 {n}^3, level 6', ct, 6, zlib.Z_DEFAULT_STRATEGY, None))
    own = {}
    for name, labels, level, strategy, key in inputs:                 # key: the map whose own dynamic fragment is the comparison
        data = labels.reshape(-1).view(torch.uint8).cpu().numpy().tobytes()
        n_bytes = len(data)
        z = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
        t0 = time.perf_counter()
        raw = z.compress(data) + z.flush()
        t_def = (time.perf_counter() - t0) * 1e3
        src = torch.zeros((len(raw) + 15) // 16 * 16, dtype=torch.uint8, device=dev)
        src[:len(raw)] = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(dev)
        out = torch.empty(n_bytes, dtype=torch.uint8, device=dev)
        one = level == 0 or strategy == zlib.Z_FIXED
        k = 1 if one else calls
        n_cand = capi.inflate_find_blocks(src.data_ptr(), len(raw), 0, 0, stream)
        say(f'{name}: {n_bytes / 2 ** 20:.0f} MiB -> {len(raw) / 2 ** 20:.2f} MiB (zlib deflate took {t_def:.0f} ms); {n_cand} candidates')
        tf = events_batched(lambda: capi.inflate_find_blocks(src.data_ptr(), len(raw), 0, 0, stream), k, windows, dev)
        row('  fnn_inflate_find_blocks (mark and scan; no positions written)', tf, f'  {len(raw) / tf[0] / 1e6:.2f} GB/s of input')
        res = []
        t = events_batched(lambda: res.append(capi.inflate_stream(src.data_ptr(), len(raw), out.data_ptr(), n_bytes, stream)), k, windows, dev)
        same = res[-1] == (0, zlib.crc32(data)) and bool((out == labels.reshape(-1).view(torch.uint8)).all())
        row('  fnn_inflate_stream', t, f'  {n_bytes / t[0] / 1e6:.2f} GB/s of output; status and CRC good, bytes equal: {same}')
        tz = wall(lambda: zlib.decompressobj(-15).decompress(raw), reps)
        verdict = 'the device call WINS' if tz[0] > t[0] else 'the device call LOSES to host zlib'
        row('  zlib inflate of the same stream (host)', tz[:3], f'  {n_bytes / tz[0] / 1e6:.2f} GB/s; {tz[0] / t[0]:.2f}x the device call\'s time: {verdict}')
        if key is not None:
            if key not in own:
                cap = capi.deflate_bound(n_bytes)
                buf = torch.empty(cap, dtype=torch.uint8, device=dev)
                n_in, _, crc_enc, _ = capi.deflate_labels_dyn(labels.data_ptr(), labels.element_size(), labels.numel(), False, buf.data_ptr(), cap, stream)
                frag = buf[:n_in].cpu().numpy().tobytes()
                starts = np.array([0] + [e for e in fio._marker_ends(frag, 0, len(frag)) if e < len(frag)], dtype=np.int64)
                own[key] = events_batched(lambda: capi.inflate_segments_dyn(buf.data_ptr(), n_in, starts, out.data_ptr(), n_bytes, stream), calls, windows, dev)
                del buf
            row('  fnn_inflate_segments_dyn on the project\'s own dynamic fragment of the map', own[key], f'  fnn_inflate_stream on zlib\'s stream takes {t[0] / own[key][0]:.1f}x that')
        del src, out, data, raw
    del inputs, ct, tiled

    wanted = list(range(1, 61))
    say(f'--- folder commands, {cases} cases of {n}^3 voxels, 60 foreground labels: every file written by zlib on the host '
        f'(compress_on_device=False); per-case wall clock with inflate_on_device=True (every file on the host, as before) and \'any\'')
    plans = {'dataset_name': 'd', 'plans_name': 'p', 'image_reader_writer': 'NibabelIO', 'configurations': {}}
    dj = {'labels': dict({'background': 0}, **{f'l{i}': i for i in wanted}), 'file_ending': '.nii.gz', 'channel_names': {'0': 'CT'}}
    with tempfile.TemporaryDirectory() as tmp:
        ref_d, pred_dir = (os.path.join(tmp, d) for d in ('ref', 'pred'))
        for d in (ref_d, pred_dir):
            os.makedirs(d)
        affine = np.diag([0.8, 0.8, 1.25, 1.0])
        for i in range(cases):
            ref = label_map(n, dev, seed=30 + i)
            pred = ref.clone()
            pred[i::7] = 0
            fio.write_label_file(ref.cpu().numpy(), os.path.join(ref_d, f'case{i}.nii.gz'), affine)
            fio.write_label_file(pred.cpu().numpy(), os.path.join(pred_dir, f'case{i}.nii.gz'), affine)
            del ref, pred
        say(f'case0 on disk: reference {os.path.getsize(os.path.join(ref_d, "case0.nii.gz")) / 2 ** 20:.2f} MiB, prediction '
            f'{os.path.getsize(os.path.join(pred_dir, "case0.nii.gz")) / 2 ** 20:.2f} MiB')
        made = {}
        for flag in (True, 'any'):
            rw = fio.NiftiIO(dev, inflate_on_device=flag)
            ev.compute_metrics_on_folder(ref_d, pred_dir, None, rw, '.nii.gz', wanted)                       # warm-up
            made[flag] = wall(lambda: ev.compute_metrics_on_folder(ref_d, pred_dir, None, rw, '.nii.gz', wanted), reps)
            row(f'compute_metrics_on_folder, inflate_on_device={flag!r}', made[flag][:3], f'  {made[flag][0] / cases:.1f} ms per case; routes {rw.inflate_stats}')
        say(f'  compute_metrics_on_folder: \'any\' takes {made["any"][0] / made[True][0]:.2f}x the time of True; equal results: {repr(made[True][3]) == repr(made["any"][3])}')
        fns, kwargs = [pp.remove_all_but_largest_component_from_segmentation], [{'labels_or_regions': wanted}]
        made = {}
        for flag in (True, 'any'):
            out_dir = os.path.join(tmp, f'post_{flag}')
            run = lambda: pp.apply_postprocessing_to_folder(pred_dir, out_dir, fns, kwargs, plans, dj, inflate_on_device=flag)   # noqa: E731
            run()                                                                                            # warm-up
            made[flag] = wall(run, reps)
            row(f'apply_postprocessing_to_folder, inflate_on_device={flag!r}', made[flag][:3], f'  {made[flag][0] / cases:.1f} ms per case')
        same = all(open(os.path.join(tmp, 'post_True', f'case{i}.nii.gz'), 'rb').read() == open(os.path.join(tmp, 'post_any', f'case{i}.nii.gz'), 'rb').read()
                   for i in range(cases))
        say(f'  apply_postprocessing_to_folder: \'any\' takes {made["any"][0] / made[True][0]:.2f}x the time of True; identical output files: {same}')


def bench_predict_files(a, dev, say, row, tmp):
    """predict_from_files_sequential and predict_from_files on a.cases generated cases under tmp (``--section predict_files``
    runs these rows alone)."""
    from fast_nnunet_amd import nnUNetPredictor
    from fast_nnunet_amd import imageio as fio
    from fast_nnunet_amd.plans import PlansManager
    from oracle.topology import UNetSpec
    from oracle.unet import synthetic_state_dict
    props = {'nibabel_stuff': {'original_affine': np.diag([0.8, 0.8, 1.25, 1.0])}}
    say(f'--- predict_from_files on {a.cases} cases of {tuple(a.case_shape)} int16 .nii.gz, toy network (patch 32 x 64 x 64), no mirroring')
    patch = (32, 64, 64)
    spec = UNetSpec('plain', 1, 3, [16, 32, 32], [(3, 3, 3)] * 3, [(1, 1, 1), (2, 2, 2), (2, 2, 2)], [2, 2, 2], [2, 2])
    pm = PlansManager({'dataset_name': 'Dataset996_Bench', 'plans_name': 'nnUNetPlans', 'transpose_forward': [0, 1, 2],
                       'transpose_backward': [0, 1, 2], 'image_reader_writer': 'NibabelIO',
                       'foreground_intensity_properties_per_channel': {},
                       'configurations': {'3d_fullres': {
                           'patch_size': list(patch), 'spacing': [1.25, 0.8, 0.8], 'normalization_schemes': ['ZScoreNormalization'],
                           'use_mask_for_norm': [False],
                           'architecture': {'network_class_name': 'PlainConvUNet', 'arch_kwargs': {}, '_kw_requires_import': []}}}})
    dj = {'labels': {'background': 0, 'a': 1, 'b': 2}, 'channel_names': {'0': 'CT'}, 'file_ending': '.nii.gz'}
    p = nnUNetPredictor(tile_step_size=0.5, use_gaussian=True, use_mirroring=False, device=dev, allow_tqdm=False, patches_per_forward=4)
    p.manual_initialization(None, pm, pm.get_configuration('3d_fullres'), [synthetic_state_dict(spec, 3)], dj, 'nnUNetTrainer', None)
    src = os.path.join(tmp, 'cases')
    os.makedirs(src)
    for i in range(a.cases):
        v = synthetic_ct(tuple(a.case_shape), 10 + i)
        hd = fio.nifti1_header_bytes(tuple(a.case_shape)[::-1], 4, props['nibabel_stuff']['original_affine'])
        with open(os.path.join(src, f'case{i}_0000.nii.gz'), 'wb') as raw, \
                gzip.GzipFile(filename='', mode='wb', compresslevel=1, fileobj=raw, mtime=0) as g:
            g.write(hd)
            g.write(v.tobytes())
    p.predict_from_files_sequential(src, os.path.join(tmp, 'warm'))
    t_seq = wall(lambda: p.predict_from_files_sequential(src, os.path.join(tmp, 'seq')), a.reps)
    t_thr = wall(lambda: p.predict_from_files(src, os.path.join(tmp, 'thr')), a.reps)
    row('predict_from_files_sequential (read, GPU, write one after the other)', t_seq[:3])
    row('predict_from_files (reader thread, writer thread)', t_thr[:3], f'  {t_seq[0] / t_thr[0]:.2f}x')
    same = all(open(os.path.join(tmp, 'seq', f'case{i}.nii.gz'), 'rb').read() == open(os.path.join(tmp, 'thr', f'case{i}.nii.gz'), 'rb').read()
               for i in range(a.cases))
    say(f'the two forms wrote identical files: {same}')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=512)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--cases', type=int, default=4)
    ap.add_argument('--case-shape', type=int, nargs=3, default=(96, 192, 192))
    ap.add_argument('--out', default=None)
    ap.add_argument('--section', choices=('all', 'reorient', 'deflate', 'masks', 'label_files', 'inflate', 'inflate_dyn', 'inflate_any', 'predict_files', 'read'), default='all')
    a = ap.parse_args()
    from fast_nnunet_amd import capi, nnUNetPredictor
    from fast_nnunet_amd import imageio as fio
    from fast_nnunet_amd.plans import PlansManager
    from oracle.topology import UNetSpec
    from oracle.unet import synthetic_state_dict

    dev = torch.device('cuda', 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    n = a.n
    lines = [f'imageio_bench: int16 volume {n}^3 ({n ** 3 * 2 / 2 ** 20:.0f} MiB of voxels, {n ** 3 * 4 / 2 ** 20:.0f} MiB as float32); '
             f'device {torch.cuda.get_device_name(dev)}',
             f'median of {a.reps} (min, max); host steps by wall clock, device steps by events on the stream']

    def say(text):
        lines.append(text)
        print(text, flush=True)

    def row(name, t, extra=''):
        say(f'{name:<66s}: {t[0]:9.2f} ms  (min {t[1]:.2f} max {t[2]:.2f}){extra}')

    if a.section == 'label_files':
        bench_label_files(n, a.reps, a.cases, dev, say, row)
        write_out(a.out or os.path.join(ROOT, 'profiles', 'r21_label_files.txt'), lines)
        return
    if a.section == 'inflate':
        bench_inflate(n, a.reps, a.cases, dev, say, row)
        write_out(a.out or os.path.join(ROOT, 'profiles', 'r25_inflate.txt'), lines)
        return
    if a.section == 'inflate_dyn':
        bench_inflate_dyn(n, a.reps, a.cases, dev, say, row)
        write_out(a.out or os.path.join(ROOT, 'profiles', 'r32_inflate_dynamic.txt'), lines)
        return
    if a.section == 'inflate_any':
        bench_inflate_any(n, a.reps, a.cases, dev, say, row)
        write_out(a.out or os.path.join(ROOT, 'profiles', 'r35_inflate_any.txt'), lines)
        return
    if a.section == 'predict_files':
        with tempfile.TemporaryDirectory() as tmp:
            bench_predict_files(a, dev, say, row, tmp)
        write_out(a.out, lines)
        return
    if a.section in ('reorient', 'deflate', 'masks'):
        {'reorient': bench_reorient, 'deflate': bench_deflate, 'masks': bench_masks}[a.section](n, a.reps, dev, say, row)
        write_out(a.out, lines)
        return

    with tempfile.TemporaryDirectory() as tmp:
        vol = synthetic_ct((n, n, n), 1)
        props = {'nibabel_stuff': {'original_affine': np.diag([0.8, 0.8, 1.25, 1.0])}}
        head = fio.nifti1_header_bytes((n, n, n), 4, props['nibabel_stuff']['original_affine'])
        f_gz, f_nii = os.path.join(tmp, 'ct_0000.nii.gz'), os.path.join(tmp, 'ct_0000.nii')
        with open(f_nii, 'wb') as f:
            f.write(head)
            f.write(vol.tobytes())
        t0 = time.perf_counter()
        with open(f_gz, 'wb') as raw, gzip.GzipFile(filename='', mode='wb', compresslevel=1, fileobj=raw, mtime=0) as g:
            g.write(head)
            g.write(vol.tobytes())
        say(f'synthetic files: .nii {os.path.getsize(f_nii) / 2 ** 20:.0f} MiB, .nii.gz {os.path.getsize(f_gz) / 2 ** 20:.0f} MiB '
            f'(gzip level 1 took {time.perf_counter() - t0:.1f} s)')

        rw = fio.NiftiIO(dev)
        for f in (f_gz, f_nii):
            tag = '.nii.gz' if f.endswith('.gz') else '.nii'
            say(f'--- this route, {tag}: file bytes -> pinned memory -> device -> fnn_decode_voxels')
            staged = rw.stage([f])
            h = staged.hdrs[0]
            row(f'{tag}: file read' + (' + inflate' if tag == '.nii.gz' else '') + ' into pinned memory (host)', wall(staged.fill, a.reps)[:3])
            raw = torch.empty(h.n_bytes, dtype=torch.uint8, device=dev)
            out = torch.empty((1, *h.shape), dtype=torch.float32, device=dev)
            t = events(lambda: raw.copy_(staged.buffers[0][:h.n_bytes], non_blocking=True), a.reps, dev)
            row(f'{tag}: upload of the voxel bytes ({h.n_bytes / 2 ** 20:.0f} MiB, pinned)', t, f'  {h.n_bytes / t[0] / 1e6:.1f} GB/s')
            t = events(lambda: capi.decode_voxels(raw.data_ptr(), h.datatype, h.byteswap, h.n_vox, h.scale, h.slope, h.inter,
                                                  out.data_ptr(), stream), a.reps, dev)
            moved = h.n_bytes + 4 * h.n_vox
            row(f'{tag}: fnn_decode_voxels int16 -> float32', t,
                f'  {moved / t[0] / 1e6:.0f} GB/s of {moved / 1e9:.2f} GB = {100 * moved / t[0] / 1e6 / (COPY_TBS * 1e3):.1f} % of {COPY_TBS} TB/s')
            if tag == '.nii.gz':
                t = events(lambda: capi.decode_voxels(raw.data_ptr(), h.datatype, h.byteswap, h.n_vox, 1, 0.5, -3.0,
                                                      out.data_ptr(), stream), a.reps, dev)
                row(f'{tag}: fnn_decode_voxels with slope and intercept (float64 arithmetic)', t, f'  {moved / t[0] / 1e6:.0f} GB/s')
                src = torch.empty(moved // 2, dtype=torch.uint8, device=dev)
                dst = torch.empty_like(src)
                t = events(lambda: dst.copy_(src), a.reps, dev)
                row(f'plain device copy moving the same bytes ({moved // 2 / 2 ** 20:.0f} MiB read + written)', t, f'  {moved / t[0] / 1e6:.0f} GB/s')
                del src, dst
            del raw, out
            row(f'{tag}: read_images, file -> float32 tensor on the device (all of the above)', wall(lambda: rw.read_images([f]), a.reps)[:3])
            if a.section == 'read':                       # these rows alone
                continue

            say(f'--- the route before, {tag}: host decode with numpy, astype(float32), upload of the float32 array')

            def host_bytes():
                if tag == '.nii.gz':
                    with gzip.open(f, 'rb') as g:
                        return g.read()
                with open(f, 'rb') as g:
                    return g.read()
            t_read = wall(host_bytes, a.reps)
            row(f'{tag}: file read' + (' + inflate' if tag == '.nii.gz' else '') + ' (host)', t_read[:3])
            blob = t_read[3]
            t_cast = wall(lambda: np.frombuffer(blob, dtype='<i2', offset=352).reshape(1, n, n, n).astype(np.float32), a.reps)
            row(f'{tag}: astype(float32) (host)', t_cast[:3])
            arr = t_cast[3]
            t_up = wall(lambda: (torch.as_tensor(arr).to(device=dev, dtype=torch.float32).contiguous(), torch.cuda.synchronize(dev)), a.reps)
            row(f'{tag}: upload of the float32 array ({arr.nbytes / 2 ** 20:.0f} MiB, pageable)', t_up[:3], f'  {arr.nbytes / t_up[0] / 1e6:.1f} GB/s')
            say(f'{tag}: sum of the three' + ' ' * 45 + f': {t_read[0] + t_cast[0] + t_up[0]:9.2f} ms')
            del blob, arr

        if a.section == 'read':
            write_out(a.out, lines)
            return

        say('--- writing a label map')
        coarse = np.random.default_rng(2).integers(0, 5, (n // 32,) * 3).astype(np.uint8)
        seg = coarse.repeat(32, 0).repeat(32, 1).repeat(32, 2)
        for name in ('seg.nii.gz', 'seg.nii'):
            t = wall(lambda: fio.write_nifti_seg(seg, os.path.join(tmp, name), props), a.reps)
            row(f'write_seg {name}, uint8 {n}^3 ({os.path.getsize(os.path.join(tmp, name)) / 2 ** 20:.1f} MiB on disk)', t[:3])
        del vol, seg

        bench_reorient(n, a.reps, dev, say, row)
        bench_deflate(n, a.reps, dev, say, row)

        bench_predict_files(a, dev, say, row, tmp)
    write_out(a.out, lines)


def write_out(out, lines):
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
