"""The torch resampling kernels (fnn_resample_torch, fnn_resample_torch_seg) on one MI355X: ms and effective GB/s -
bytes the pass has to move (input read once + output written once) over time - against the ~6.3 TB/s float4 copy rate
of MI355X HBM, for

* the export of the headline workload: 61 heads of fp16 logits from its network grid (spacing 2.0 x 0.977 x 0.977) to a
  512^3 cropped grid of a case scanned at 1.25 x 0.78 x 0.78 (network grid 320 x 410 x 410);
* a 2-channel fp32 image the other way (512^3 -> 320 x 410 x 410), and along a separate axis;
* a 118-label int16 segmentation the same way, under both rules;

and the default family (fnn_resample, order 1 and order 3; for the segmentation order 1 per label through
DevicePreprocessor.resample_seg) on the same shapes, for scale;

* labels from logits (--section labels, or all): per family the fused pass (fnn_resample_labels: logits read once,
  labels written) next to the two-step pair it replaces, timed in the same run - the resampling step alone
  (fnn_resample order 1 / fnn_resample_torch) and that step followed by fnn_argmax_labels - with the bytes each moves and
  the time those bytes take at the copy rate.

usage (repo root, GPU box): python tools/resample_torch_bench.py [--n 512] [--heads 61] [--reps 5] [--section all|labels|resample] [--out FILE]
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
    ap.add_argument('--section', choices=['all', 'labels', 'resample'], default='all')
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
        return ms

    def say(text):
        lines.append(text)
        print(text, flush=True)

    def label_runs(x, new_shape):
        """labels [new_shape] from logits x: the fused pass against the resampling step alone and the two-step pair."""
        from fast_nnunet_amd import nnUNetPredictor
        from fast_nnunet_amd.plans import PlansManager
        from oracle.topology import UNetSpec
        from oracle.unet import synthetic_state_dict
        H = x.shape[0]
        spec = UNetSpec('plain', 1, H, [8, 16, 16], [(3, 3, 3)] * 3, [(1, 1, 1), (2, 2, 2), (1, 2, 2)], [2, 2, 2], [2, 2])
        pm = PlansManager({'dataset_name': 'bench', 'plans_name': 'nnUNetPlans', 'configurations': {'3d_fullres': {
            'patch_size': [16, 16, 32], 'architecture': {'network_class_name': 'PlainConvUNet', 'arch_kwargs': {},
                                                         '_kw_requires_import': []}}}})
        dj = {'labels': {('background' if i == 0 else f'c{i}'): i for i in range(H)}, 'channel_names': {'0': 'CT'},
              'file_ending': '.nii.gz'}
        p = nnUNetPredictor(use_mirroring=False, device=dev, allow_tqdm=False, patches_per_forward=2)
        p.manual_initialization(None, pm, pm.get_configuration('3d_fullres'), [synthetic_state_dict(spec, 1)], dj, 'nnUNetTrainer', None)
        engine = p._engine                                   # fnn_argmax_labels takes its label rule from an engine
        engine.set_label_rule(None, uint16=H > 256)
        half = x.dtype == torch.half
        dt = capi.FNN_OUT_F16 if half else capi.FNN_OUT_F32
        out = torch.empty((H, *new_shape), dtype=x.dtype, device=dev)
        labels = torch.empty(new_shape, dtype=torch.int16 if H > 256 else torch.uint8, device=dev)
        fused = torch.empty_like(labels)
        n_out = labels.numel()
        b_in, b_out, b_lab = x.numel() * x.element_size(), out.numel() * out.element_size(), n_out * labels.element_size()
        tag = f'labels from logits {H} x {tuple(x.shape[1:])} -> {tuple(new_shape)}'
        for family, fam_id, reps in (('torch', capi.FNN_RESAMPLE_TORCH, a.reps), ('default', capi.FNN_RESAMPLE_DEFAULT, 2)):
            if family == 'torch':
                step1 = lambda: capi.resample_torch(x.data_ptr(), x.shape, new_shape, None, half, out.data_ptr(), stream)
            else:
                step1 = lambda: capi.resample(x.data_ptr(), x.shape, new_shape, 1, None, half, out.data_ptr(), stream)

            def pair():
                step1()
                engine.argmax_labels(out.data_ptr(), dt, H, n_out, labels.data_ptr(), stream)
            t_step = report(f'{tag}, {family}: resampling step alone', *timed(step1, reps, dev), b_in + b_out)
            t_pair = report(f'{tag}, {family}: two steps (+ fnn_argmax_labels)', *timed(pair, reps, dev), b_in + 2 * b_out + b_lab)
            t_fused = report(f'{tag}, {family}: fused (fnn_resample_labels)',
                             *timed(lambda: capi.resample_labels(x.data_ptr(), half, x.shape, new_shape, fam_id, None, None, H,
                                                                 fused.data_ptr(), H > 256, stream), a.reps, dev), b_in + b_lab)
            same = bool(torch.equal(fused, labels))
            say(f'    {family}: fused {t_fused:.2f} ms = {t_step / t_fused:.2f}x faster than the resampling step alone, '
                f'{t_pair / t_fused:.2f}x than the two steps; floor of its {(b_in + b_lab) / 1e9:.2f} GB at the copy rate '
                f'{(b_in + b_lab) / COPY_TBS / 1e9:.2f} ms; labels equal the two-step labels: {same}; kernel {capi.op_last_kernels()}')

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
    if a.section != 'labels':
        image_runs(f'logits fp16 {H} x {net_grid} -> {raw_grid}', logits, raw_grid, 1)
    if a.section != 'resample':
        label_runs(logits, raw_grid)
    del logits
    torch.cuda.empty_cache()
    if a.section == 'labels':
        return finish(lines, a.out)
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
    finish(lines, a.out)


def finish(lines, out):
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
