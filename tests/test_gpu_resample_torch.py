"""The torch resampling family (``resample_torch_fornnunet`` plans) on a real MI355X against torch's own operator on the
CPU (tests/resample_torch_ref.py, pinned to the reference by tests/test_resample_torch_cpu.py).

Gates
* fp32 images: per case B = max |F.interpolate(x) - F.interpolate(x.double())| on the CPU, the float32 operator's own
  distance from exact arithmetic; the kernel must stay within max(2 B, 4 * 6e-8 * max|x|) of F.interpolate(x) - twice the
  operator's own error for a correct float32 implementation whose coordinate rounding differs, the project's resampling
  tolerance as the floor.
* fp16: within one fp16 step of the float32 yardstick rounded to fp16, everywhere (which data: see the test).
* segmentations: equal to the yardstick except at its near-ties (two best fp16 scores within 0.5; |score - 0.5| <= 2^-20
  for the memefficient rule), where the label must be one of its two best; near-ties at most 2 % of a case, asserted on
  the yardstick before anything is compared (``resample_torch_ref.check_labels``).
* export: the probabilities may move by half the logits' movement (sum_j |d softmax_i / d z_j| = 2 p_i (1 - p_i) <= 1/2),
  i.e. half an fp16 step of the largest logit, plus 1e-6 for the float32 softmax; labels may differ from the yardstick's
  only where its two best fp16 logits are within two fp16 steps (each may sit one step off).
* the whole chain through the network: the share of differing labels the project already allows the default family's
  chain (5e-3: the network input differs in its last float32 bits and a few near-tie voxels flip) - same network, same
  driver, only the interpolator differs.
Measured figures are printed with -s."""
import numpy as np
import pytest
import torch

import resample_torch_ref as rt
from golden_cases import toy_unet_spec
from oracle import preprocess as opre
from oracle import sliding_window as osw
from oracle.unet import synthetic_state_dict

pytestmark = pytest.mark.gpu

TORCH_FN = 'resample_torch_fornnunet'
TORCH_KW = {'is_seg': False, 'force_separate_z': None, 'memefficient_seg_resampling': False,
            'separate_z_anisotropy_threshold': 3}
DEV = torch.device('cuda', 0)

# (C, in shape, out shape, separate axis)
FIXED = [
    (2, (14, 42, 38), (19, 57, 33), None),
    (1, (130, 111, 95), (97, 150, 64), None),
    (3, (20, 24, 28), (40, 48, 56), None),             # exactly 2x
    (2, (31, 40, 25), (13, 16, 10), None),             # 0.4
    (1, (12, 33, 30), (12, 71, 30), None),             # two unchanged axes
    (2, (1, 40, 36), (1, 57, 80), None),               # a size-1 axis that stays
    (2, (1, 17, 23), (2, 30, 11), None),               # a size-1 axis that is enlarged
    (1, (2, 9, 1), (1, 19, 2), None),
    (2, (9, 48, 52), (14, 77, 61), 0),
    (2, (40, 7, 52), (61, 12, 33), 1),
    (3, (44, 38, 6), (30, 70, 13), 2),
    (1, (10, 30, 30), (10, 45, 41), 0),                # separate axis unchanged
    # rows of 64 and more output voxels over at most 512 input voxels: the row-staged kernel
    (3, (9, 11, 150), (7, 14, 200), None),
    (1, (7, 9, 70), (11, 6, 70), None),                # z unchanged
    (2, (6, 5, 300), (5, 7, 131), None),
    (2, (9, 30, 70), (14, 41, 100), 0),
    (2, (20, 7, 90), (31, 12, 64), 1),
    (3, (20, 24, 40), (13, 37, 77), 2),
    (2, (3, 4, 300), (2, 5, 600), None),               # several output voxels per lane and row
    (1, (3, 4, 600), (4, 3, 700), None),               # a longer input row: back to one thread per voxel
]


def random_cases(n=24):
    out = []
    for i in range(n):
        rng = np.random.default_rng(4000 + i)
        shape = [int(v) for v in rng.integers(5, 41, 3)]
        new = [max(1, int(round(s * rng.uniform(0.4, 2.2)))) for s in shape]
        kind, axis = i % 6, None
        if kind == 1:                                  # an unchanged axis
            a = int(rng.integers(0, 3)); new[a] = shape[a]
        elif kind == 2:                                # a size-1 axis
            a = int(rng.integers(0, 3)); shape[a] = 1; new[a] = int(rng.integers(1, 3))
        elif kind >= 3:
            axis = kind - 3
        out.append((1 + i % 3, tuple(shape), tuple(new), axis))
    return out


IMAGE_CASES = FIXED + random_cases()


def _ids(c):
    return f"{c[0]}x{'x'.join(map(str, c[1]))}->{'x'.join(map(str, c[2]))}" + ('' if c[3] is None else f'_sep{c[3]}')


def _pp():
    from fast_nnunet_amd.preprocess import DevicePreprocessor
    return DevicePreprocessor(DEV)


def _spacings(axis):
    """current / new spacings that make determine_do_sep_z_and_axis pick `axis` (None: isotropic)."""
    cur = [1.0, 1.0, 1.0]
    if axis is not None:
        cur[axis] = 5.0
    return cur, [1.0, 1.0, 1.0]


def _gpu_resample(x, new_shape, axis, kw=TORCH_KW):
    cur, new = _spacings(axis)
    return _pp().resample(x.to(DEV), new_shape, cur, new, kw, TORCH_FN)


def f16_steps(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """Distance of two fp16 tensors in representable values (+0 and -0 coincide)."""
    def key(t):
        bits = t.contiguous().view(torch.int16).to(torch.int32)
        return torch.where(bits < 0, -(bits & 0x7fff), bits)
    return (key(a) - key(b)).abs()


@pytest.mark.parametrize('case', IMAGE_CASES, ids=_ids)
def test_fp32_images_against_torch(case):
    C, shape, new_shape, axis = case
    x = torch.randn(C, *shape, generator=torch.Generator().manual_seed(sum(shape) + C)) * 3 + 1
    want = rt.resample(x, new_shape, axis)
    B = float((want.double() - rt.resample(x.double(), new_shape, axis)).abs().max())
    gate = max(2 * B, 4 * 6e-8 * float(x.abs().max()))
    got = _gpu_resample(x, new_shape, axis)
    assert got.dtype == torch.float32 and tuple(got.shape) == (C, *new_shape)
    err = float((got.cpu() - want).abs().max())
    print(f'[{_ids(case)}] max|err| {err:.3g}  B {B:.3g}  gate {gate:.3g}  ratio {err / gate:.3f}')
    assert err <= gate


def _fp16_input(case, signed):
    C, shape, _, _ = case
    x = torch.randn(C, *shape, generator=torch.Generator().manual_seed(sum(shape) + 7 * C)) * 4
    return (x if signed else x.abs() + 2).half()


@pytest.mark.parametrize('case', IMAGE_CASES, ids=_ids)
def test_fp16_logits_against_torch(case):
    """Within one fp16 step of the float32 yardstick rounded to fp16, everywhere.  Trilinear cases run signed data: the
    kernel blends in the rounding order of torch's 3-D kernel and gives its float32 bits.  torch's 2-D kernel (the plane
    of a separate-axis case) sums its four products in an order that changes with the shape and with the number of CPU
    threads, so its own float32 results differ from run to run in the last bit - far more than one fp16 step where a
    value crosses zero.  The separate-axis cases therefore run data bounded away from zero here, where a float32 step
    is a small fraction of an fp16 step, and signed data in the next test."""
    C, shape, new_shape, axis = case
    x = _fp16_input(case, signed=axis is None)
    want = rt.resample(x.float(), new_shape, axis).half()
    got = _gpu_resample(x, new_shape, axis)
    assert got.dtype == torch.half and tuple(got.shape) == (C, *new_shape)
    steps = f16_steps(got.cpu(), want)
    print(f'[{_ids(case)}] fp16: unequal share {float((steps != 0).float().mean()):.5f}, max steps {int(steps.max())}')
    assert int(steps.max()) <= 1


@pytest.mark.parametrize('case', [c for c in IMAGE_CASES if c[3] is not None], ids=_ids)
def test_fp16_signed_logits_along_a_separate_axis(case):
    """Signed fp16 data through the separate-axis path: the fp16 result is the float32 result rounded once, and the
    float32 result may sit 2 B from torch's (the fp32 gate), so |got - want| <= 2 B + one fp16 step of want."""
    C, shape, new_shape, axis = case
    x = _fp16_input(case, signed=True)
    want32 = rt.resample(x.float(), new_shape, axis)
    B = float((want32.double() - rt.resample(x.double(), new_shape, axis)).abs().max())
    want = want32.half()
    got = _gpu_resample(x, new_shape, axis).cpu()
    step = torch.pow(2.0, torch.floor(torch.log2(want.float().abs().clamp_min(2.0 ** -14))) - 10)
    excess = ((got.float() - want.float()).abs() - step).max()
    steps = f16_steps(got, want)
    print(f'[{_ids(case)}] signed fp16: unequal share {float((steps != 0).float().mean()):.5f}, max steps {int(steps.max())}, '
          f'beyond one step {float(excess):.3g} (2 B = {2 * B:.3g})')
    assert float(excess) <= 2 * B


def test_identity_and_dtype_rules():
    x = torch.randn(2, 9, 10, 11, generator=torch.Generator().manual_seed(1))
    assert torch.equal(_gpu_resample(x, (9, 10, 11), None).cpu(), x)
    # an unchanged axis is the identity along it: every x slice equals the slice resampled on its own
    got = _gpu_resample(x, (9, 15, 7), None).cpu()
    for i in range(9):
        assert torch.equal(got[:, i:i + 1], _gpu_resample(x[:, i:i + 1].contiguous(), (1, 15, 7), None).cpu())
    # integer input is resampled as float32, like the default family
    assert _gpu_resample((x * 10).to(torch.int32), (5, 15, 7), None).dtype == torch.float32


def test_refusals():
    from fast_nnunet_amd import capi
    pp = _pp()
    x = torch.zeros(1, 4, 4, 4, device=DEV)
    out = torch.zeros(1, 6, 6, 6, device=DEV)
    iso = [1.0] * 3
    with pytest.raises(RuntimeError, match='resample_magic'):
        pp.resample(x, (6, 6, 6), iso, iso, {}, 'resample_magic')
    with pytest.raises(NotImplementedError):
        pp.resample(x, (6, 6, 6), iso, iso, dict(TORCH_KW, mode='bicubic'), TORCH_FN)
    with pytest.raises(NotImplementedError):
        capi.resample_torch(x.data_ptr(), x.shape, (6, 6, 6), None, False, out.data_ptr(), mode='nearest')
    with pytest.raises(NotImplementedError):
        capi.resample_torch(x.data_ptr(), x.shape, (6, 6, 6), 0, False, out.data_ptr(), aniso_axis_mode='linear')
    with pytest.raises(AssertionError):                                   # host pointer
        capi.resample_torch(x.cpu().data_ptr(), x.shape, (6, 6, 6), None, False, out.data_ptr())
    with pytest.raises(AssertionError):
        capi.resample_torch(x.data_ptr(), (1, 4, 4, 0), (6, 6, 6), None, False, out.data_ptr())
    assert pp.resample(x, (6, 6, 6), iso, iso, {}, 'no_resampling_data_or_seg_to_shape') is x


# ---- segmentations -----------------------------------------------------------------------------------------------
LABELS = {
    'few': (tuple(range(4)), (4, 5, 4)),
    'sparse': ((0, 3, 7, 200, 1000), (4, 5, 4)),                         # non-contiguous values, beyond int8
    'many118': (tuple(range(118)), (7, 8, 7)),
}
# in shape, out shape, separate axis: non-dyadic ratios (at exactly 2x the midpoints score exactly 0.5)
SEG_SHAPES = [
    ((14, 42, 38), (19, 57, 33), None),
    ((40, 36, 44), (27, 47, 30), None),
    ((9, 48, 52), (13, 67, 41), 0),
    ((44, 10, 40), (59, 7, 53), 1),
    ((38, 46, 8), (51, 33, 11), 2),
]
SEG_SHAPES_118 = [((48, 56, 52), (67, 75, 43), None), ((12, 70, 64), (17, 93, 81), 0)]


def seg_cases():
    out = []
    for name in LABELS:
        for shp in (SEG_SHAPES_118 if name == 'many118' else SEG_SHAPES):
            for memeff in (False, True):
                out.append((name, *shp, memeff))
    return out


def _seg_id(c):
    return f"{c[0]}_{'x'.join(map(str, c[1]))}->{'x'.join(map(str, c[2]))}" + ('' if c[3] is None else f'_sep{c[3]}') + \
        ('_memeff' if c[4] else '_argmax')


def make_seg(name, shape):
    values, coarse = LABELS[name]
    return rt.blobby_labels(shape, values, seed=len(values) + sum(shape), coarse=coarse)


@pytest.mark.parametrize('case', seg_cases(), ids=_seg_id)
def test_segmentations_against_torch(case):
    name, shape, new_shape, axis, memeff = case
    seg = make_seg(name, shape)
    values, scores = rt.seg_scores(seg, new_shape, axis, memeff)
    rt.check_labels(rt.labels_from_scores(values, scores, memeff), values, scores, memeff)     # the cap, on the yardstick alone
    cur, new = _spacings(axis)
    kw = dict(TORCH_KW, is_seg=True, memefficient_seg_resampling=memeff)
    got = _pp().resample_seg(torch.from_numpy(seg), new_shape, cur, new, kw, TORCH_FN)
    assert got.dtype == torch.int16 and tuple(got.shape) == (1, *new_shape)
    share, diff = rt.check_labels(got.cpu().numpy(), values, scores, memeff)
    print(f'[{_seg_id(case)}] {len(values)} labels present, near-tie share {share:.4f}, labels off the yardstick {diff}')
    if name == 'many118':
        assert len(values) >= 100


def test_segmentation_channels_and_identity():
    a, b = make_seg('few', (14, 20, 18)), make_seg('sparse', (14, 20, 18))
    both = torch.from_numpy(np.concatenate([a, b]))
    iso = [1.0] * 3
    kw = dict(TORCH_KW, is_seg=True)
    pp = _pp()
    got = pp.resample_seg(both, (19, 27, 15), iso, iso, kw, TORCH_FN).cpu()
    assert torch.equal(got[0:1], pp.resample_seg(both[0:1], (19, 27, 15), iso, iso, kw, TORCH_FN).cpu())
    assert torch.equal(got[1:2], pp.resample_seg(both[1:2], (19, 27, 15), iso, iso, kw, TORCH_FN).cpu())
    assert torch.equal(pp.resample_seg(both, (14, 20, 18), iso, iso, kw, TORCH_FN).cpu(), both)


# ---- through the preprocessor, the export and the predictor ------------------------------------------------------------
IP = {'0': {'mean': 100.0, 'std': 250.0, 'percentile_00_5': -400.0, 'percentile_99_5': 800.0}}


def _plans(spacing_cfg, transpose, family, patch=(16, 16, 32), memeff=False):
    """family 'torch': what the reference's resample_with_torch planners write; 'default': no resampling entries at all."""
    from fast_nnunet_amd.plans import PlansManager
    cfg = {'patch_size': list(patch), 'spacing': list(spacing_cfg), 'normalization_schemes': ['CTNormalization'],
           'use_mask_for_norm': [False],
           'architecture': {'network_class_name': 'PlainConvUNet', 'arch_kwargs': {}, '_kw_requires_import': []}}
    if family == 'torch':
        for key, is_seg in (('data', False), ('seg', True), ('probabilities', False)):
            cfg[f'resampling_fn_{key}'] = TORCH_FN
            cfg[f'resampling_fn_{key}_kwargs'] = dict(TORCH_KW, is_seg=is_seg, memefficient_seg_resampling=memeff)
    pm = PlansManager({'dataset_name': 'Dataset998_TorchRes', 'plans_name': 'nnUNetPlans_torchres',
                       'transpose_forward': list(transpose), 'transpose_backward': [int(i) for i in np.argsort(transpose)],
                       'foreground_intensity_properties_per_channel': IP, 'configurations': {'3d_fullres': cfg}})
    return pm, pm.get_configuration('3d_fullres')


def _raw(seed=11, shape=(34, 40, 52)):
    rng = np.random.default_rng(seed)
    raw = (rng.standard_normal((1, *shape)) * 300 + 150).astype(np.float32)
    raw[:, :3] = 0; raw[:, :, -5:] = 0; raw[:, :, :, :2] = 0
    return raw


def _axis(cur, new):
    from fast_nnunet_amd.preprocess import determine_do_sep_z_and_axis
    do_sep, axis = determine_do_sep_z_and_axis(None, cur, new, 3)
    return axis if do_sep else None


CHAIN = [((1.5, 0.8, 0.8), (1.0, 1.0, 1.0), (0, 1, 2)),
         ((0.8, 4.0, 0.8), (1.0, 2.0, 1.0), (1, 0, 2))]                  # anisotropic after the transpose: separate axis 0


@pytest.mark.parametrize('memeff', [False, True], ids=['argmax', 'memeff'])
@pytest.mark.parametrize('spacing_raw,spacing_cfg,transpose', CHAIN)
def test_run_case_npy_on_a_torch_resampling_configuration(spacing_raw, spacing_cfg, transpose, memeff):
    from fast_nnunet_amd.preprocess import compute_new_shape
    pm, cm = _plans(spacing_cfg, transpose, 'torch', memeff=memeff)
    raw = _raw()
    prev = np.transpose(make_seg('few', [raw.shape[1 + i] for i in transpose])[0], np.argsort(transpose))[None]
    assert prev.shape == raw.shape
    got, got_seg, props = _pp().run_case_npy(raw, prev, {'spacing': list(spacing_raw)}, pm, cm)
    data, bbox, before = opre.preprocess_case(raw, transpose, ['CTNormalization'], IP)
    sp_t = [spacing_raw[i] for i in transpose]
    new_shape = compute_new_shape(data.shape[1:], sp_t, spacing_cfg)
    axis = _axis(sp_t, spacing_cfg)
    assert (axis is not None) == (transpose == (1, 0, 2))
    x = torch.from_numpy(np.ascontiguousarray(data))
    want = rt.resample(x, new_shape, axis)
    B = float((want.double() - rt.resample(x.double(), new_shape, axis)).abs().max())
    gate = max(2 * B, 4 * 6e-8 * float(x.abs().max()))
    err = float((got.cpu() - want).abs().max())
    print(f'image: max|err| {err:.3g} gate {gate:.3g}')
    assert tuple(got.shape) == (1, *new_shape) and err <= gate
    seg_t = np.transpose(prev, (0, *[1 + i for i in transpose]))[(slice(None), *[slice(lo, hi) for lo, hi in bbox])]
    values, scores = rt.seg_scores(np.ascontiguousarray(seg_t), new_shape, axis, memeff)
    assert got_seg.dtype == torch.int16 and tuple(got_seg.shape) == (1, *new_shape)
    share, diff = rt.check_labels(got_seg.cpu().numpy(), values, scores, memeff)
    print(f'previous-stage segmentation: near-tie share {share:.4f}, labels off the yardstick {diff}')


def _predictor(pm, cm, heads=3, patch=(16, 16, 32)):
    from fast_nnunet_amd import nnUNetPredictor
    spec = toy_unet_spec(1, heads)
    dj = {'labels': {('background' if i == 0 else f'c{i}'): i for i in range(heads)}, 'channel_names': {'0': 'CT'},
          'file_ending': '.nii.gz'}
    p = nnUNetPredictor(tile_step_size=0.5, use_gaussian=True, use_mirroring=False, perform_everything_on_device=True,
                        device=DEV, verbose=False, allow_tqdm=False, patches_per_forward=3)
    p.manual_initialization(None, pm, cm, [synthetic_state_dict(spec, 17)], dj, 'nnUNetTrainer', None)
    return p, spec


def _f16_step_of(v: float) -> float:
    return 2.0 ** (max(np.floor(np.log2(max(abs(v), 2.0 ** -14))), -14) - 10)


def _labels_with_margin(got, back16, bbox, before, tb, heads):
    """got (raw grid) against the label rule on the yardstick's fp16 logits `back16` [heads, cropped]: differences only
    where the yardstick's two best logits are within two fp16 steps, and then one of those two."""
    top = back16.float().topk(2, dim=0)
    step = torch.pow(2.0, torch.floor(torch.log2(top.values.abs().max(0).values.clamp_min(2.0 ** -14))) - 10)
    tie = ((top.values[0] - top.values[1]) <= 2 * step).numpy()
    want = opre.revert_labels(top.indices[0].numpy().astype(np.uint8), bbox, before, tb, heads - 1)
    second = opre.revert_labels(top.indices[1].numpy().astype(np.uint8), bbox, before, tb, heads - 1)
    tie_raw = opre.revert_labels(tie.astype(np.uint8), bbox, before, tb, heads - 1).astype(bool)
    differ = got != want
    assert not (differ & ~tie_raw).any(), f'{int((differ & ~tie_raw).sum())} labels differ away from near-ties'
    assert (got[differ] == second[differ]).all()
    return float(differ.mean()), float(tie.mean())


@pytest.mark.parametrize('spacing_raw,spacing_cfg,transpose', CHAIN)
def test_export_of_logits_on_a_torch_resampling_configuration(spacing_raw, spacing_cfg, transpose):
    from fast_nnunet_amd.preprocess import compute_new_shape
    pm, cm = _plans(spacing_cfg, transpose, 'torch')
    p, spec = _predictor(pm, cm)
    pp = _pp()
    raw = _raw(12)
    _, _, props = pp.run_case_npy(raw, None, {'spacing': list(spacing_raw)}, pm, cm)
    data, bbox, before = opre.preprocess_case(raw, transpose, ['CTNormalization'], IP)
    sp_t = [spacing_raw[i] for i in transpose]
    net_shape = compute_new_shape(data.shape[1:], sp_t, spacing_cfg)
    tb = [int(i) for i in np.argsort(transpose)]
    g = torch.Generator().manual_seed(5)
    smooth = torch.nn.functional.interpolate(torch.randn(1, spec.num_heads, 5, 6, 7, generator=g), net_shape,
                                             mode='trilinear')[0]
    logits = (smooth * 6 + torch.randn(spec.num_heads, *net_shape, generator=g) * 0.3).half()
    axis = _axis(spacing_cfg, sp_t)
    back16 = rt.resample(logits.float(), data.shape[1:], axis).half()

    got_logits = pp.resample_logits_to_cropped_shape(logits.to(DEV), pm, cm, props)
    assert got_logits.dtype == torch.half and tuple(got_logits.shape) == tuple(back16.shape)
    steps = f16_steps(got_logits.cpu(), back16)
    print(f'resampled logits: unequal share {float((steps != 0).float().mean()):.5f}, max steps {int(steps.max())}')
    assert int(steps.max()) <= 1

    got = pp.convert_predicted_logits_to_segmentation_with_correct_shape(logits.to(DEV), p, pm, cm, props).cpu().numpy()
    assert got.shape == raw.shape[1:]
    differ, tie = _labels_with_margin(got, back16, bbox, before, tb, spec.num_heads)
    print(f'labels: {differ:.5f} differ, near-tie share {tie:.5f}')

    seg2, probs = pp.convert_predicted_logits_to_segmentation_and_probabilities(logits.to(DEV), p, pm, cm, props)
    want_seg2, want_probs = opre.export_with_probabilities(back16.float().numpy(), bbox, before, tb, spec.num_heads - 1)
    gate = 0.5 * _f16_step_of(float(back16.float().abs().max())) + 1e-6
    err = float(np.abs(probs.cpu().numpy() - want_probs).max())
    print(f'probabilities: max|err| {err:.3g} gate {gate:.3g}')
    assert err <= gate
    _labels_with_margin(seg2.cpu().numpy(), back16, bbox, before, tb, spec.num_heads)


@pytest.mark.parametrize('spacing_raw,spacing_cfg,transpose', CHAIN)
def test_predict_single_npy_array_on_a_torch_resampling_plan(spacing_raw, spacing_cfg, transpose):
    from fast_nnunet_amd.preprocess import compute_new_shape
    pm, cm = _plans(spacing_cfg, transpose, 'torch')
    p, spec = _predictor(pm, cm)
    raw = _raw()
    got = p.predict_single_npy_array(raw, {'spacing': list(spacing_raw)})
    assert got.dtype == np.uint8 and got.shape == raw.shape[1:]
    data, bbox, before = opre.preprocess_case(raw, transpose, ['CTNormalization'], IP)
    sp_t = [spacing_raw[i] for i in transpose]
    tb = [int(i) for i in np.argsort(transpose)]
    new_shape = compute_new_shape(data.shape[1:], sp_t, spacing_cfg)
    net_in = rt.resample(torch.from_numpy(np.ascontiguousarray(data)), new_shape, _axis(sp_t, spacing_cfg))
    logits = osw.sliding_window_logits(lambda t: p.forward_patches(t).cpu(), net_in, (16, 16, 32), spec.num_heads,
                                       accum='fp16')
    back = rt.resample(logits.float(), data.shape[1:], _axis(spacing_cfg, sp_t)).half().float()
    lab = osw.logits_to_labels(back).numpy().astype(np.uint8)
    want = opre.revert_labels(lab, bbox, before, tb, spec.num_heads - 1)
    mismatch = float((got != want).mean())
    print(f'label mismatch {mismatch:.5f}')
    assert mismatch < 5e-3 and len(np.unique(got)) >= 2
    seg2, probs = p.predict_single_npy_array(raw, {'spacing': list(spacing_raw)}, save_or_return_probabilities=True)
    assert probs.dtype == np.float32 and probs.shape == (spec.num_heads, *raw.shape[1:])
    assert np.abs(probs.sum(0) - 1).max() < 1e-5 and (seg2 != got).mean() < 1e-4
    # the cubic of the default family gives another network input: the plan's choice reaches the kernels
    pm_d, cm_d = _plans(spacing_cfg, transpose, 'default')
    pp = _pp()
    a, _, _ = pp.run_case_npy(raw, None, {'spacing': list(spacing_raw)}, pm, cm)
    b, _, _ = pp.run_case_npy(raw, None, {'spacing': list(spacing_raw)}, pm_d, cm_d)
    assert a.shape == b.shape and not torch.equal(a, b)


# ---- a default plan computes what it computed ---------------------------------------------------------------------------
class _OldCM:
    """A configuration as the preprocessor saw it before it looked at function names: kwargs only."""
    def __init__(self, cm):
        self.spacing, self.normalization_schemes, self.use_mask_for_norm = cm.spacing, cm.normalization_schemes, cm.use_mask_for_norm
        self.resampling_fn_data_kwargs = cm.resampling_fn_data_kwargs
        self.resampling_fn_seg_kwargs = {'is_seg': True, 'order': 1, 'order_z': 0, 'force_separate_z': None}
        self.resampling_fn_probabilities_kwargs = cm.resampling_fn_probabilities_kwargs


@pytest.mark.parametrize('spacing_raw,spacing_cfg,transpose', CHAIN)
def test_a_default_plan_gives_the_same_bits_as_the_old_path(spacing_raw, spacing_cfg, transpose):
    from fast_nnunet_amd import capi
    from fast_nnunet_amd.preprocess import DEFAULT_RESAMPLING_FN, determine_do_sep_z_and_axis
    pm, cm = _plans(spacing_cfg, transpose, 'default')
    assert cm.resampling_fn_data_name == cm.resampling_fn_seg_name == cm.resampling_fn_probabilities_name == DEFAULT_RESAMPLING_FN
    pp = _pp()
    raw = _raw(13)
    prev = np.transpose(make_seg('few', [raw.shape[1 + i] for i in transpose])[0], np.argsort(transpose))[None]
    a, a_seg, props = pp.run_case_npy(raw, prev, {'spacing': list(spacing_raw)}, pm, cm)
    b, b_seg, props_b = pp.run_case_npy(raw, prev, {'spacing': list(spacing_raw)}, pm, _OldCM(cm))
    assert torch.equal(a, b) and torch.equal(a_seg, b_seg) and props == props_b
    # ... and as fnn_resample called directly on the preprocessor's input
    sp_t = [spacing_raw[i] for i in transpose]
    data, _, _ = opre.preprocess_case(raw, transpose, ['CTNormalization'], IP)
    x = torch.from_numpy(np.ascontiguousarray(data)).to(DEV)
    kw = cm.resampling_fn_data_kwargs
    via = pp.resample(x, a.shape[1:], sp_t, spacing_cfg, kw, DEFAULT_RESAMPLING_FN)
    assert torch.equal(via, pp.resample(x, a.shape[1:], sp_t, spacing_cfg, kw))
    do_sep, axis = determine_do_sep_z_and_axis(None, sp_t, spacing_cfg)
    direct = torch.empty_like(via)
    capi.resample(x.data_ptr(), x.shape, a.shape[1:], 3, axis if do_sep else None, False, direct.data_ptr())
    torch.cuda.synchronize()
    assert torch.equal(via, direct)
    # the export: logits -> cropped grid -> labels, with and without the names
    p, spec = _predictor(pm, cm)
    logits = (torch.randn(spec.num_heads, *a.shape[1:], generator=torch.Generator().manual_seed(3)) * 4).half().to(DEV)
    la = pp.resample_logits_to_cropped_shape(logits, pm, cm, props)
    lb = pp.resample_logits_to_cropped_shape(logits, pm, _OldCM(cm), props)
    assert torch.equal(la, lb)
    do_sep, axis = determine_do_sep_z_and_axis(None, spacing_cfg, sp_t)
    direct = torch.empty_like(la)
    capi.resample(logits.data_ptr(), logits.shape, la.shape[1:], 1, axis if do_sep else None, True, direct.data_ptr())
    torch.cuda.synchronize()
    assert torch.equal(la, direct)
    sa = pp.convert_predicted_logits_to_segmentation_with_correct_shape(logits, p, pm, cm, props)
    sb = pp.convert_predicted_logits_to_segmentation_with_correct_shape(logits, p, pm, _OldCM(cm), props)
    assert torch.equal(sa, sb)
