"""Engines come and go: every device buffer, pinned buffer, stream and event of an engine belongs to a member that frees it
(csrc/owned.h), and ``fnn_destroy`` is a device synchronisation and a ``delete``.  One cycle here builds a predictor, takes it
through every path that makes the engine create a resource of its own, and closes the engine; three cycles in one process
give the same bits each time, the host-volume results are the resident volume's, and a second engine that was created before
the first one closed and is used after it still gives those bits - no owner is shared, and none is freed twice or left behind
for the next engine to trip over.

The smallest shapes that still give more patches than one batch (80 patches of 16 x 16 x 32 at batch 4), so that the pipes, their
arenas and their events come into being.  No memory figure is asserted: free device memory is device-wide on a shared card
(tools/engine_lifecycle.py prints it, profiles/r27_engine_lifecycle.txt keeps one run)."""
import os

import numpy as np
import pytest
import torch

from golden_cases import DATASET_JSONS, toy_unet_spec
from oracle.unet import synthetic_state_dict
from test_gpu_predictor import _bits, _predictor

pytestmark = pytest.mark.gpu

SPEC, PATCH, BATCH = toy_unet_spec(1, 3), (16, 16, 32), 4


def _inputs():
    g = torch.Generator().manual_seed(27)
    return {'vol': torch.randn((1, 40, 48, 80), generator=g), 'small': torch.randn((1, 12, 20, 20), generator=g),
            'patches': torch.randn((5, 1, *PATCH), generator=g)}


def new_predictor():
    """Three heads = the three regions of the rule set: fnn_set_label_rule makes the engine's label_order."""
    return _predictor(SPEC, PATCH, [synthetic_state_dict(SPEC, 270)], batch=BATCH, dataset_json=DATASET_JSONS['regions'])


def use_engine(p, x):
    """Every call that makes the engine create something of its own -> {name: the result's bits}."""
    out = {}
    # the pipelined gather path: feat / featss / featssh, both integer tables, the pipes with their arenas and events
    out['resident'] = _bits(p.predict_sliding_window_return_logits(x['vol'].cuda()))
    # a host volume: vol_tmp, the copy stream and its event pool; pageable through the staging ring (many tiles), pinned by DMA
    old = os.environ.get('FNN_UPLOAD_SLAB_BYTES')
    os.environ['FNN_UPLOAD_SLAB_BYTES'] = str(65536)
    try:
        out['pageable'] = _bits(p.predict_sliding_window_return_logits(x['vol']))
    finally:
        if old is None:
            os.environ.pop('FNN_UPLOAD_SLAB_BYTES', None)
        else:
            os.environ['FNN_UPLOAD_SLAB_BYTES'] = old
    out['pinned'] = _bits(p.predict_sliding_window_return_logits(x['vol'].pin_memory()))
    # mirroring into fp32 accumulators: acc, patch_buf
    p.use_mirroring, p.allowed_mirroring_axes, p.accumulate_in = True, (0, 1, 2), 'fp32'
    out['mirror_fp32'] = _bits(p.predict_sliding_window_return_logits(x['vol'].cuda()))
    p.use_mirroring, p.allowed_mirroring_axes, p.accumulate_in = False, None, 'fp16'
    # smaller than the patch: vol_pad
    out['small'] = _bits(p.predict_sliding_window_return_logits(x['small'].cuda()))
    # region labels: label_order
    out['labels'] = p.predict_segmentation_from_preprocessed_data(x['vol'].cuda()).cpu().numpy()
    # patches from and to host memory: vol_tmp, out_tmp, the origins table
    logits = torch.empty((x['patches'].shape[0], SPEC.num_heads, *PATCH), dtype=torch.float32)
    p._engine.forward_patches(x['patches'].data_ptr(), x['patches'].shape[0], logits.data_ptr(),
                              stream=torch.cuda.current_stream().cuda_stream)
    out['patches'] = logits.numpy().view(np.uint32).copy()
    # profiling: the event pairs
    p._engine.set_profiling(True)
    try:
        out['profiled'] = _bits(p.predict_sliding_window_return_logits(x['vol'].cuda()))
        assert p._engine.profile().total_ms > 0
    finally:
        p._engine.set_profiling(False)
    return out


def one_cycle(x):
    p = new_predictor()
    try:
        return use_engine(p, x)
    finally:
        p._engine.close()


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), k


def test_three_engine_lifecycles_give_the_same_bits_and_share_no_owner():
    x = _inputs()
    survivor = new_predictor()                     # created before the first engine is closed, used after the last one is
    first = one_cycle(x)
    assert len(np.unique(first['labels'])) >= 2 and np.isfinite(first['resident'].view(np.float16).astype(np.float32)).all()
    for k in ('pageable', 'pinned', 'profiled'):
        assert np.array_equal(first[k], first['resident']), k
    assert not np.array_equal(first['mirror_fp32'], first['resident'])
    for _ in range(2):
        _same(one_cycle(x), first)
    try:
        _same(use_engine(survivor, x), first)
    finally:
        survivor._engine.close()
    survivor._engine.close()                       # an empty handle: nothing happens
