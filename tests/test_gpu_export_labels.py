"""``fnn_resample_labels`` on a real MI355X: labels on the cropped grid straight from the logits of the network grid.

1. Identity: the labels equal, in every voxel, those of the two-step route on the same input - ``capi.resample`` (order 1)
   or ``capi.resample_torch`` writes the resampled logits, ``fnn_argmax_labels`` applies the rule.  Both families, fp16 and
   fp32 logits, the argmax rule over all heads and the region rule (order [3, 1, 2]) over the first three.  The shapes are
   the smallest that reach every branch, and every instantiation of the two kernels (dtype x which axes interpolate) is
   named by a case.
2. An independent yardstick on the CPU: ``oracle.resample.resample_data(order=1)`` / ``tests/resample_torch_ref.py`` and
   numpy's argmax; labels equal wherever the yardstick's two largest fp16 logits differ by more than 2 fp16 steps; at most
   0.02 of a case is excluded (the near-tie cap of the segmentation resampling tests; with logits standard_normal * 4 the
   default-family yardstick leaves out 0.0013 - 0.0126 of these shapes).
3. Through the predictor: ``fused_label_export`` True and False give equal label maps, and the fused kernel ran.
4. The fused route allocates no resampled tensor: its peak stays under half of heads * n_out * 2 bytes where the two-step
   route's reaches it.
5. Refusals raise before any launch."""
import numpy as np
import pytest
import torch

import resample_torch_ref as rt
from golden_cases import DATASET_JSONS, toy_unet_spec
from oracle import resample as ores
from oracle.unet import synthetic_state_dict

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda', 0)
REGION_ORDER = [3, 1, 2]
FAMILIES = ['default', 'torch']

# name: (heads, in shape, out shape, separate axis)
CASES = {
    'up': (5, (9, 7, 11), (13, 10, 17), None),
    'down': (3, (20, 24, 28), (12, 15, 17), None),
    'axis0_unchanged': (5, (9, 7, 11), (9, 12, 15), None),
    'size1_axis': (4, (1, 8, 9), (1, 13, 11), None),
    'size1_axis_enlarged': (4, (1, 8, 9), (2, 13, 11), None),
    'sep0_kept': (5, (6, 14, 12), (6, 21, 19), 0),
    'sep0_changed': (5, (6, 14, 12), (9, 21, 19), 0),
    'sep1_kept': (5, (14, 6, 12), (21, 6, 19), 1),
    'sep1_changed': (5, (14, 6, 12), (21, 9, 19), 1),
    'sep2_kept': (5, (14, 12, 6), (21, 19, 6), 2),
    'sep2_changed': (5, (14, 12, 6), (21, 19, 4), 2),
    'long_rows': (3, (5, 6, 45), (7, 9, 70), None),
    'heads67': (67, (5, 6, 7), (8, 9, 11), None),
    # the remaining combinations of interpolating axes
    'only_axis0': (5, (6, 7, 8), (9, 7, 8), None),
    'only_axis1': (5, (6, 7, 8), (6, 10, 8), None),
    'only_axis2': (5, (6, 7, 8), (6, 7, 11), None),
    'only_the_pick': (5, (6, 7, 8), (9, 7, 8), 0),
    'plateau_integer_ratios': (3, (4, 6, 8), (8, 3, 16), None),
    'plateau_odd_ratios': (3, (7, 6, 9), (10, 11, 13), None),
}
YARDSTICK_CASES = ['up', 'down', 'sep0_changed', 'long_rows', 'heads67']


def _mask(shape, new_shape, axis):
    return sum(1 << a for a in range(3) if shape[a] != new_shape[a] and a != axis)


def _logits(name, dtype, heads=None, shape=None):
    h, s, _, _ = CASES[name]
    rng = np.random.default_rng(sorted(CASES).index(name) + 77)
    x = (rng.standard_normal((heads or h, *(shape or s))) * 4).astype(np.float32)
    if name.startswith('plateau'):
        # blocks held at the channel's maximum and minimum: the blend's weights meet equal taps at the clip bounds
        hi, lo = np.float32(9.123457), np.float32(-8.765432)
        x[:, :2, :3, :4] = hi
        x[:, -2:, -2:, -3:] = lo
        x[1, 1:3, 2:5, 3:7] = hi
    return torch.from_numpy(x).to(dtype)


@pytest.fixture(scope='module')
def engine():
    """A 3-head engine: fnn_argmax_labels, the second step of the yardstick, takes its label rule from an engine."""
    from fast_nnunet_amd import nnUNetPredictor
    from fast_nnunet_amd.plans import PlansManager
    spec = toy_unet_spec(1, 3)
    pm = PlansManager({'dataset_name': 'Dataset997_ExportLabels', 'plans_name': 'nnUNetPlans',
                       'configurations': {'3d_fullres': {'patch_size': [16, 16, 32], 'architecture': {
                           'network_class_name': 'PlainConvUNet', 'arch_kwargs': {}, '_kw_requires_import': []}}}})
    p = nnUNetPredictor(use_mirroring=False, device=DEV, allow_tqdm=False, patches_per_forward=2)
    p.manual_initialization(None, pm, pm.get_configuration('3d_fullres'), [synthetic_state_dict(spec, 3)],
                            DATASET_JSONS['labels3'], 'nnUNetTrainer', None)
    return p._engine


def _order_on_device(order):
    return None if order is None else torch.tensor(order, dtype=torch.int32, device=DEV)


def two_step(engine, lg, new_shape, family, axis, order, u16):
    """The parent's route: resampled logits [heads, *new_shape], then fnn_argmax_labels."""
    from fast_nnunet_amd import capi
    half = lg.dtype == torch.half
    out = torch.empty((lg.shape[0], *new_shape), dtype=lg.dtype, device=DEV)
    if family == 'torch':
        capi.resample_torch(lg.data_ptr(), lg.shape, new_shape, axis, half, out.data_ptr())
    else:
        capi.resample(lg.data_ptr(), lg.shape, new_shape, 1, axis, half, out.data_ptr())
    engine.set_label_rule(order, uint16=u16)
    labels = torch.empty(new_shape, dtype=torch.int16 if u16 else torch.uint8, device=DEV)
    engine.argmax_labels(out.data_ptr(), capi.FNN_OUT_F16 if half else capi.FNN_OUT_F32, lg.shape[0], out[0].numel(),
                         labels.data_ptr())
    torch.cuda.synchronize(DEV)
    return labels.cpu().numpy()


def fused(lg, new_shape, family, axis, order, u16):
    from fast_nnunet_amd import capi
    dev_order = _order_on_device(order)
    labels = torch.empty(new_shape, dtype=torch.int16 if u16 else torch.uint8, device=DEV)
    capi.resample_labels(lg.data_ptr(), lg.dtype == torch.half, lg.shape, new_shape,
                         capi.FNN_RESAMPLE_TORCH if family == 'torch' else capi.FNN_RESAMPLE_DEFAULT, axis,
                         None if order is None else dev_order.data_ptr(), lg.shape[0], labels.data_ptr(), u16)
    torch.cuda.synchronize(DEV)
    return labels.cpu().numpy(), capi.op_last_kernels()


def _same_labels(engine, x, new_shape, family, axis, u16=False):
    """Both rules on x: argmax over all heads, regions over the first three.  -> the fused argmax labels."""
    lg = x.to(DEV).contiguous()
    got, _ = fused(lg, new_shape, family, axis, None, u16)
    want = two_step(engine, lg, new_shape, family, axis, None, u16)
    assert got.dtype == want.dtype and np.array_equal(got, want), f'{int((got != want).sum())} argmax labels differ'
    lg3 = lg[:3].contiguous()
    got3, _ = fused(lg3, new_shape, family, axis, REGION_ORDER, False)
    want3 = two_step(engine, lg3, new_shape, family, axis, REGION_ORDER, False)
    assert np.array_equal(got3, want3), f'{int((got3 != want3).sum())} region labels differ'
    return got, got3


# ---- 1. identity with the two-step route ------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [torch.half, torch.float32], ids=['f16', 'f32'])
@pytest.mark.parametrize('family', FAMILIES)
@pytest.mark.parametrize('name', list(CASES))
def test_labels_equal_the_two_step_route(engine, name, family, dtype):
    heads, shape, new_shape, axis = CASES[name]
    x = _logits(name, dtype)
    got, got3 = _same_labels(engine, x, new_shape, family, axis)
    assert len(np.unique(got)) >= 2 and len(np.unique(got3)) >= 2
    # ... and the kernel that ran is the instantiation of this dtype and these interpolating axes
    _, names = fused(x.to(DEV), new_shape, family, axis, None, False)
    assert names == [f"export_labels_{family}_kernel<{'f16' if dtype == torch.half else 'f32'},{_mask(shape, new_shape, axis)}>"]


def test_every_instantiation_is_named_by_a_case():
    masks = {_mask(s, n, a) for _, s, n, a in CASES.values()}
    assert masks == set(range(8))


@pytest.mark.parametrize('family', FAMILIES)
def test_uint16_labels_for_258_heads(engine, family):
    x = (torch.randn(258, 3, 4, 5, generator=torch.Generator().manual_seed(9)) * 4).half().to(DEV)
    got, _ = fused(x, (5, 6, 7), family, None, None, True)
    want = two_step(engine, x, (5, 6, 7), family, None, None, True)
    assert got.dtype == np.int16 and np.array_equal(got, want) and int(got.max()) > 255


@pytest.mark.parametrize('dtype', [torch.half, torch.float32], ids=['f16', 'f32'])
@pytest.mark.parametrize('family', FAMILIES)
def test_duplicated_heads_the_first_index_wins(engine, family, dtype):
    one = _logits('up', dtype, heads=1)
    got, got3 = _same_labels(engine, one.repeat(5, 1, 1, 1), CASES['up'][2], family, None)
    assert (got == 0).all()                                     # every voxel an exact tie of all heads
    # regions: the last head above the threshold paints, i.e. REGION_ORDER[-1] wherever the shared value is above it
    assert set(np.unique(got3)) == {0, REGION_ORDER[-1]}


@pytest.mark.parametrize('value', [float('nan'), float('inf'), float('-inf')], ids=['nan', 'inf', '-inf'])
@pytest.mark.parametrize('dtype', [torch.half, torch.float32], ids=['f16', 'f32'])
@pytest.mark.parametrize('family', FAMILIES)
@pytest.mark.parametrize('name', ['up', 'axis0_unchanged', 'sep0_changed'])
def test_one_special_logit(engine, name, family, dtype, value):
    """One NaN in the interior (the first-NaN rule), and infinities in the interior and in the high corner: there the
    default family's upper tap has weight 0 (inf * 0 = NaN, formed by both routes), a single-tap axis has none."""
    heads, shape, new_shape, axis = CASES[name]
    x = _logits(name, dtype)
    x[2, shape[0] // 2, shape[1] // 2, shape[2] // 2] = value
    if value == value:
        x[1, -1, -1, -1] = value
    got, _ = _same_labels(engine, x, new_shape, family, axis)
    if value != value:
        assert (got == 2).sum() >= 8                            # the NaN's neighbourhood takes head 2


# ---- 2. an independent yardstick on the CPU ---------------------------------------------------------------------------
@pytest.mark.parametrize('family', FAMILIES)
@pytest.mark.parametrize('name', YARDSTICK_CASES)
def test_labels_against_the_cpu_yardstick(name, family):
    heads, shape, new_shape, axis = CASES[name]
    x = _logits(name, torch.half)
    if family == 'torch':
        back = rt.resample(x.float(), new_shape, axis).half()
    else:
        back = torch.from_numpy(ores.resample_data(x.numpy(), new_shape, axis=axis, order=1, do_separate_z=axis is not None))
        assert back.dtype == torch.half
    top = back.float().topk(2, dim=0)
    step = torch.pow(2.0, torch.floor(torch.log2(top.values.abs().max(0).values.clamp_min(2.0 ** -14))) - 10)
    tie = ((top.values[0] - top.values[1]) <= 2 * step).numpy()
    share = float(tie.mean())
    print(f'{name} {family}: near-tie share {share:.4f}')
    assert share <= 0.02
    want = back.float().numpy().argmax(0)
    got, _ = fused(x.to(DEV), new_shape, family, axis, None, False)
    differ = got != want
    print(f'{name} {family}: labels off the yardstick {int(differ.sum())} of {differ.size}')
    assert not (differ & ~tie).any(), f'{int((differ & ~tie).sum())} labels differ away from near-ties'
    assert (got[differ] == top.indices[1].numpy()[differ]).all()


# ---- 3. through the predictor ------------------------------------------------------------------------------------------
IP = {'0': {'mean': 100.0, 'std': 250.0, 'percentile_00_5': -400.0, 'percentile_99_5': 800.0}}
TORCH_KW = {'is_seg': False, 'force_separate_z': None, 'memefficient_seg_resampling': False,
            'separate_z_anisotropy_threshold': 3}
# family: (raw spacing, configuration spacing, transpose_forward)
CHAIN = {'default': ((0.8, 4.0, 0.8), (1.0, 2.0, 1.0), (1, 0, 2)),     # anisotropic after the transpose: separate axis 0
         'torch': ((1.5, 0.8, 0.8), (1.0, 1.0, 1.0), (0, 1, 2))}


def _plans(family, spacing_cfg, transpose):
    from fast_nnunet_amd.plans import PlansManager
    cfg = {'patch_size': [16, 16, 32], 'spacing': list(spacing_cfg), 'normalization_schemes': ['CTNormalization'],
           'use_mask_for_norm': [False],
           'architecture': {'network_class_name': 'PlainConvUNet', 'arch_kwargs': {}, '_kw_requires_import': []}}
    if family == 'torch':
        for key, is_seg in (('data', False), ('seg', True), ('probabilities', False)):
            cfg[f'resampling_fn_{key}'] = 'resample_torch_fornnunet'
            cfg[f'resampling_fn_{key}_kwargs'] = dict(TORCH_KW, is_seg=is_seg)
    pm = PlansManager({'dataset_name': 'Dataset997_ExportLabels', 'plans_name': 'nnUNetPlans',
                       'transpose_forward': list(transpose), 'transpose_backward': [int(i) for i in np.argsort(transpose)],
                       'foreground_intensity_properties_per_channel': IP, 'configurations': {'3d_fullres': cfg}})
    return pm, pm.get_configuration('3d_fullres')


def _predictor(pm, cm, heads, dataset_json, fused_label_export):
    from fast_nnunet_amd import nnUNetPredictor
    p = nnUNetPredictor(tile_step_size=0.5, use_gaussian=True, use_mirroring=False, device=DEV, allow_tqdm=False,
                        patches_per_forward=3, fused_label_export=fused_label_export)
    p.manual_initialization(None, pm, cm, [synthetic_state_dict(toy_unet_spec(1, heads), 17)], dataset_json, 'nnUNetTrainer', None)
    return p


@pytest.mark.parametrize('rule', ['argmax', 'regions'])
@pytest.mark.parametrize('family', FAMILIES)
def test_predictor_gives_the_same_labels_either_way(family, rule):
    from fast_nnunet_amd import capi
    spacing_raw, spacing_cfg, transpose = CHAIN[family]
    pm, cm = _plans(family, spacing_cfg, transpose)
    dj = dict(DATASET_JSONS['regions'], regions_class_order=REGION_ORDER) if rule == 'regions' else DATASET_JSONS['labels3']
    rng = np.random.default_rng(11)
    raw = (rng.standard_normal((1, 34, 40, 52)) * 300 + 150).astype(np.float32)
    raw[:, :3] = 0; raw[:, :, -5:] = 0; raw[:, :, :, :2] = 0
    props = {'spacing': list(spacing_raw)}
    got = _predictor(pm, cm, 3, dj, True).predict_single_npy_array(raw, dict(props))
    names = capi.op_last_kernels()
    want = _predictor(pm, cm, 3, dj, False).predict_single_npy_array(raw, dict(props))
    assert got.shape == raw.shape[1:] and got.dtype == want.dtype == np.uint8
    assert np.array_equal(got, want) and len(np.unique(got)) >= 2
    mask = 6 if family == 'default' else 7                     # the separate axis of the default chain is a pick
    assert names == [f'export_labels_{family}_kernel<f16,{mask}>']


# ---- 4. no intermediate tensor -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('family', FAMILIES)
def test_the_fused_route_allocates_no_resampled_logits(family):
    heads, net, cropped = 16, (24, 24, 24), (64, 64, 64)
    pm, cm = _plans(family, (1.0, 1.0, 1.0), (0, 1, 2))
    dj = {'labels': {('background' if i == 0 else f'c{i}'): i for i in range(heads)}, 'channel_names': {'0': 'CT'},
          'file_ending': '.nii.gz'}
    props = {'spacing': [0.375, 0.375, 0.375], 'shape_before_cropping': cropped,
             'shape_after_cropping_and_before_resampling': cropped, 'bbox_used_for_cropping': [[0, n] for n in cropped]}
    from fast_nnunet_amd.preprocess import DevicePreprocessor
    pp = DevicePreprocessor(DEV)
    logits = (torch.randn(heads, *net, generator=torch.Generator().manual_seed(2)) * 4).half().to(DEV)
    resampled_bytes = heads * int(np.prod(cropped)) * 2
    out, rise = {}, {}
    for fused_route in (True, False):
        p = _predictor(pm, cm, heads, dj, fused_route)
        torch.cuda.synchronize(DEV)
        torch.cuda.reset_peak_memory_stats(DEV)
        before = torch.cuda.memory_allocated(DEV)
        out[fused_route] = pp.convert_predicted_logits_to_segmentation_with_correct_shape(logits, p, pm, cm, props)
        torch.cuda.synchronize(DEV)
        rise[fused_route] = torch.cuda.max_memory_allocated(DEV) - before
    print(f'{family}: peak rise fused {rise[True]} B, two-step {rise[False]} B, resampled logits {resampled_bytes} B')
    assert rise[False] >= resampled_bytes                      # otherwise the comparison shows nothing
    assert rise[True] < resampled_bytes // 2
    assert torch.equal(out[True], out[False])


# ---- 5. refusals -------------------------------------------------------------------------------------------------------
def test_refusals():
    from fast_nnunet_amd import capi
    lg = torch.zeros((3, 4, 5, 6), dtype=torch.half, device=DEV)
    labels = torch.full((5, 6, 7), 77, dtype=torch.uint8, device=DEV)
    order = _order_on_device(REGION_ORDER)
    lib = capi.load_library()
    shape, new = (capi.C.c_int64 * 4)(3, 4, 5, 6), (capi.C.c_int64 * 3)(5, 6, 7)

    def call(logits=lg.data_ptr(), dtype=capi.FNN_OUT_F16, shape=shape, new=new, family=capi.FNN_RESAMPLE_DEFAULT, axis=-1,
             order_ptr=None, n=3, labels_ptr=labels.data_ptr(), label_dtype=capi.FNN_LABEL_U8):
        capi.check(lib.fnn_resample_labels(logits, dtype, shape, new, family, axis, order_ptr, n, labels_ptr, label_dtype, 0), lib)

    call()                                                       # the arguments the refusals below vary are fine
    labels.fill_(77)
    host = np.zeros(3 * 4 * 5 * 6, np.float16)
    host_order = np.asarray(REGION_ORDER, np.int32)
    for kw, exc in [(dict(logits=None), AssertionError), (dict(labels_ptr=None), AssertionError),
                    (dict(shape=None), AssertionError), (dict(new=None), AssertionError),
                    (dict(logits=host.ctypes.data), AssertionError),                       # host pointers
                    (dict(order_ptr=host_order.ctypes.data), AssertionError),
                    (dict(shape=(capi.C.c_int64 * 4)(0, 4, 5, 6)), AssertionError),         # heads < 1
                    (dict(shape=(capi.C.c_int64 * 4)(3, 4, 0, 6)), AssertionError),
                    (dict(new=(capi.C.c_int64 * 3)(5, 0, 7)), AssertionError),
                    (dict(axis=3), AssertionError), (dict(axis=-2), AssertionError),
                    (dict(order_ptr=order.data_ptr(), n=2), AssertionError),                # one entry per head
                    (dict(family=2), NotImplementedError),
                    (dict(dtype=2), AssertionError), (dict(label_dtype=2), AssertionError)]:
        with pytest.raises(exc) as e:
            call(**kw)
        assert str(e.value), kw                                  # each with a message
    torch.cuda.synchronize(DEV)
    assert (labels == 77).all()                                  # nothing was launched
    # more than 256 heads cannot be told apart in uint8
    big = torch.zeros((257, 2, 2, 2), dtype=torch.half, device=DEV)
    with pytest.raises(AssertionError):
        capi.resample_labels(big.data_ptr(), True, big.shape, (3, 3, 3), capi.FNN_RESAMPLE_TORCH, None, None, 257,
                             labels.data_ptr(), False)
