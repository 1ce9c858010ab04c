"""tests/test_gpu_stem_fused_exact.py without a GPU: every committed (case, mode) is what it claims to be - patches inside a
sentinel surround at non-zero origins, unambiguous norms, exact sums, exact statistics -, every case names the kernel the
launch rules (restated here) give its shape, the over-grid cases have more work units than the persistent grid restated for
them with ranges across planes and items, and mutants of the reference change the expected bits of a committed case."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import body_ref as B  # noqa: E402
import conv_ref as R  # noqa: E402
import test_gpu_stem_fused_exact as G  # noqa: E402

EX = (slice(None), slice(None), None, None, None)


def _flips_of(case, mode):
    return case.flips if mode == case.modes[0] else case.flips[:1]


def _windows(vol, origins, flips, dims):
    return np.stack([R.stem_window(vol if vol.ndim == 4 else vol[i], o, flips, dims) for i, o in enumerate(origins)]).astype(np.float64)


def _check_placement(vol, origins, dims):
    """every patch has volume on every side, origins are non-zero and differ, everything outside the patches is a sentinel"""
    own = vol.ndim == 5
    assert (origins > 0).all() and len({tuple(o) for o in origins}) == len(origins)
    assert (origins + np.array(dims) < np.array(vol.shape[-3:])).all()
    outside = np.ones(vol.shape, bool)
    for i, o in enumerate(origins):
        sl = tuple(slice(a, a + p) for a, p in zip(o, dims))
        outside[((i,) if own else ()) + (slice(None),) + sl] = False
    assert outside.any() and (vol[outside] >= G.SENTINEL / 2).all()
    if own:
        assert len({float(vol[i, 0, 0, 0, 0]) for i in range(len(origins))}) == len(origins)        # another sentinel per item


# ---- every committed case ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case,mode', [(c, m) for c in G.STEM_CASES for m in c.modes], ids=lambda v: v.id if isinstance(v, G.Case) else v)
def test_committed_stem_case_is_exact(case, mode):
    for flips in _flips_of(case, mode):
        d, y16 = G.stem_reference(case.id, mode, flips)
        _check_placement(d['vol'], d['origins'], case.dims)
        assert d['vol'].ndim == 4                                  # one volume for every item, as the sliding window has it
        x = _windows(d['vol'], d['origins'], flips, case.dims)
        assert y16.shape == (case.n, case.cout, *case.dims)
        if mode != 'round':
            assert np.array_equal(B.h16(x), x) and R.fits_exact(x, d['w'], d['bias'])
            assert not np.array_equal(x[0], x[1])                  # different content per item
            assert (d['w'] != 0).all()                             # every tap
        if mode == 'stats':
            assert R.stats_fit_exact(y16)
        if mode == 'round':
            h = B.h16(x)
            assert np.array_equal(G._bits(y16), G._bits(h[:, [co % case.c for co in range(case.cout)]] + 0.0))
            down = np.where(np.abs(h) > np.abs(x), np.nextafter(h.astype(np.float16), np.float16(0)).astype(np.float64), h)
            step = np.spacing(np.abs(down).astype(np.float16)).astype(np.float64)
            ties = np.abs(x) - np.abs(down) == step / 2
            assert ties.sum() >= 100 and (ties & (np.abs(x) < 2.0 ** -14)).sum() >= 10 and (ties & (np.abs(x) > 2048)).sum() >= 10
            near = (np.abs(x) != np.abs(down)) & ~ties & (np.abs(np.abs(x) - np.abs(down) - step / 2) <= np.abs(x) * 2.0 ** -22)
            assert near.sum() >= 200                               # one fp32 ulp either side of a tie
            assert not np.array_equal(G._bits(down), G._bits(h))   # truncation is another answer


FUSED = G.FUSED_STEM_CASES + G.FUSED_TCONV_CASES


@pytest.mark.parametrize('case,mode', [(c, m) for c in FUSED for m in c.modes], ids=lambda v: v.id if isinstance(v, G.Case) else v)
def test_committed_fused_case_is_unambiguous_and_exact(case, mode):
    for flips in _flips_of(case, mode):
        d, amb, y16 = G.fused_reference(case.id, mode, flips)
        a, amb4 = G.fused_staged(case, d, margin=4.0)
        assert amb == 0 and amb4 == 0
        assert y16.shape == (case.n, 16, *case.dims) and a.shape[1] == (16 if case.kind == 'fstem' else 32)
        if case.kind == 'fstem':
            _check_placement(d['vol'], d['origins'], case.dims)
            x = _windows(d['vol'], d['origins'], flips, case.dims)
            # the stem's sums and its statistics are exact: stage16's bracket of (scale, shift) holds for what the device sums
            assert R.fits_exact(x, d['sw'], d['sbias']) and R.stats_fit_exact(d['stem'])
            if mode in ('dense', 'stats'):
                assert d['vol'].ndim == 5 and all(np.array_equal(x[0], x[i]) for i in range(1, case.n))
            else:
                assert d['vol'].ndim == 4 and not np.array_equal(x[0], x[1])
        else:
            assert R.stage_params(d['low'], d['lnorm'], margin=4.0)[3] == 0 if d['lnorm'] is not None else True
            if not mode.startswith('readout'):
                assert R.fits_exact(R.stage16(d['low'], d['lnorm'], d['lslope'])[0], d['tw'].swapaxes(0, 1), d['tbias'])
        if mode.startswith('readout'):
            assert not np.array_equal(a[0], a[1]) and (np.abs(d['w']).reshape(16, -1).sum(1) == 1).all()
        else:
            assert R.fits_exact(a, d['w'], d['bias'])
        if mode == 'dense':
            norms = [(d['stem'], d['norm'], 0)] if case.kind == 'fstem' else [(d['low'], d['lnorm'], 0), (d['skip'], d['snorm'], 2)]
            for x, norm, off in norms:
                sc_h, sh_h, _, _ = R.stage_params(x, norm)
                S, H = G._targets(x.shape[1], off)
                assert (sc_h == S).all() and (sh_h == H).all()
            assert (d['w'] != 0).all()
        if mode == 'stats':
            assert R.stats_fit_exact(y16)


def test_readout_modes_reach_every_tap_and_both_chunks():
    for case in FUSED:
        modes = [m for m in case.modes if m.startswith('readout')]
        if not modes:
            continue
        taps = int(np.prod(case.k))
        seen = set()
        for m in modes:
            w = G._one_hot_consumer(32 if case.kind == 'ftconv' else 16, case.k, chunk=int(m == 'readout-skip'), tap0=G.READOUT_TAP0[m])
            co, ci, t = np.nonzero(w.reshape(16, -1, taps))
            seen |= {(int(c) // 16, int(tt)) for c, tt in zip(ci, t)}
            assert sorted(ci % 16) == list(range(16))              # every channel of the chunk
        chunks = {0, 1} if 'readout-skip' in modes else {0}
        assert seen >= {(ch, t) for ch in {0} for t in range(taps)} and {ch for ch, _ in seen} == chunks, case.id


# ---- the launch rules, restated ----------------------------------------------------------------------------------------
def _row_shape(dims):
    return dims[2] in G.ROW_W and dims[1] % 4 == 0 and dims[1] >= 8


def _stem_kernel(case, store):
    """launch_stem_mfma's rule (conv3d_thin.hip) with stem_row_ok (conv3d_row.hip)"""
    D, H, W = case.dims
    slots = -(-D // 16) * -(-H // 8) * -(-W // 8)                  # stem_mfma_stats_slots
    off = 'FNN_NO_ROW' in case.knobs or 'FNN_NO_STEM_ROW' in case.knobs
    if not off and case.c == 1 and case.k == G.K133 and case.cout == 16 and _row_shape(case.dims) and D * G.pick_strips(H)[0] <= slots:
        return f'stem_row_kernel<{W // 16},{store}>'
    if case.c == 1 and case.k[1:] == (3, 3) and case.cout in (16, 32) and 'FNN_NO_STEM1' not in case.knobs:
        return f'stem_mfma1_kernel<{case.cout // 16},{case.k[0]}>'
    return 'stem_mfma_kernel'


def test_every_case_names_the_kernels_the_launch_rules_give_its_shape():
    for c in G.STEM_CASES:
        assert c.kernels == (_stem_kernel(c, 1),), c.id
    for c in G.FUSED_STEM_CASES:                                   # row_choose, else thin_choose (conv_choose's order)
        row = 'FNN_NO_ROW' not in c.knobs and 'FNN_NO_STEM_ROW' not in c.knobs and c.k == G.K133 and _row_shape(c.dims)
        consumer = f'conv_row_stem_kernel<{c.dims[2] // 16}>' if row else f'conv_thin_kernel<{c.k[0]},1,1,1,2>'
        assert c.kernels == (_stem_kernel(c, 0), consumer), c.id
    for c in G.FUSED_TCONV_CASES:
        row = 'FNN_NO_ROW' not in c.knobs and c.c == 32 and c.tstride == (1, 2, 2) and _row_shape(c.dims)
        taps = int(np.prod(c.tstride))
        assert taps in (4, 8) and c.c in (16, 32) and all(c.dims[i] % c.tstride[i] == 0 for i in range(3))
        assert c.kernels == (f'conv_row_kernel<{c.dims[2] // 16},2,1>' if row else f'conv_thin_kernel<1,2,2,{taps},2>',), c.id
    named = set().union(*(c.kernels for c in G.CASES))
    assert G.REQUIRED_KERNELS <= named
    # the strip forms of the row shapes: one strip, two groups, the fallback beyond 64 rows, a seam
    assert [G.pick_strips(h) for h in G.ROW_H] == [(1, 8), (1, 12), (1, 68), (2, 36)]
    # the tile forms end ragged on every axis and have more than one tile per axis
    for c in G.CASES:
        if c.kernels[-1].startswith(('stem_mfma', 'conv_thin')) and c.id != 'ftconv-row-96-no-row':
            tile = (16, 8, 8) if c.kind == 'stem' else (4, 8, 8)
            assert all(d % t != 0 for d, t in zip(c.dims, tile)) and all(d > t or (t == 16 and c.k[0] == 1) for d, t in zip(c.dims, tile)), c.id
    # every knob a case depends on is read per call (FNN_STEM_WPC, FNN_ROW_WPC, FNN_ROW1_WPC3 are read once per process)
    assert {k for c in G.CASES for k in c.knobs} <= set(G.KNOBS)
    twin = G.BY_ID[G.ROW_TWIN['ftconv-row-96-no-row']]
    assert twin.dims == G.BY_ID['ftconv-row-96-no-row'].dims and twin.kernels != G.BY_ID['ftconv-row-96-no-row'].kernels
    assert all(np.array_equal(G.fused_tconv_data(twin, 'ident')[k], G.fused_tconv_data(G.BY_ID['ftconv-row-96-no-row'], 'ident')[k])
               for k in ('low', 'skip', 'tw', 'w'))


def _ranges(total, nwg):
    """a persistent workgroup's units: [total g / nwg, total (g + 1) / nwg) (conv3d_row.hip; fnn_xcd_tile only permutes g)"""
    return [(total * g // nwg, total * (g + 1) // nwg) for g in range(nwg)]


def _crossings(n, planes, nwg):
    inside = items = 0
    for a, b in _ranges(n * planes, nwg):
        inside += b - a >= 2
        items += b - a >= 2 and a // planes != (b - 1) // planes
    return inside, items


def test_over_grid_cases_have_more_units_than_their_persistent_grid():
    seen = set()
    for c in G.CASES:
        if not c.grid:
            continue
        name = c.kernels[0 if c.kind == 'stem' else -1].split('<')[0]
        assert G.PERSISTENT_WGS[name] == c.grid < G.units(c), c.id
        seen.add(name)
        if name != 'conv_thin_kernel':                             # row forms: one strip per plane; ranges of two units cross planes and an item
            assert G.pick_strips(c.dims[1])[0] == 1
            inside, items = _crossings(c.n, c.dims[0], c.grid)
            assert inside >= 1 and items >= 1, c.id
    assert seen == set(G.PERSISTENT_WGS)
    assert _crossings(2, 1035, 2048) == (22, 0) and _crossings(4, 200, 768) == (32, 0)       # the counts that cross no item
    assert G.units(G.BY_ID['fstem-thin-1']) == 540 and G.units(G.BY_ID['ftconv-thin-8-c32']) == 540


# ---- sensitivity: mutants of the reference ---------------------------------------------------------------------------------
def _differs(y, z):
    return not np.array_equal(G._bits(y), G._bits(z))


def _conv64(a, w, bias, pad):
    b = None if bias is None else torch.from_numpy(np.asarray(bias, np.float64))
    return B.h16(F.conv3d(torch.from_numpy(np.ascontiguousarray(a, np.float64)), torch.from_numpy(np.asarray(w, np.float64)), b, padding=pad).numpy()) + 0.0


def test_mutant_shift_applied_to_the_consumers_zero_padding():
    case = G.BY_ID['fstem-row-64-8']
    d, _, y16 = G.fused_reference(case.id, 'dense', case.flips[0])
    a = G.fused_staged(case, d)[0]
    _, sh_h, _, _ = R.stage_params(d['stem'], d['norm'])
    fill = R.act16(sh_h, d['slope'])                               # what a zero voxel becomes when the shift reaches it
    pad = ((0, 0), (0, 0), (0, 0), (1, 1), (1, 1))
    border = np.pad(np.zeros(a.shape[2:]), pad[2:], constant_values=1.0)
    assert not _differs(y16, _conv64(np.pad(a, pad), d['w'], d['bias'], 0))
    assert _differs(y16, _conv64(np.pad(a, pad) + border[None, None] * fill[EX], d['w'], d['bias'], 0))


def test_mutant_sentinel_read_where_the_patchs_zero_padding_belongs():
    for cid in ('stem-row-64-8', 'stem1-1-3'):
        case = G.BY_ID[cid]
        d, y16 = G.stem_reference(cid, 'ident', G.FLIPS[0])
        pad = [(k - 1) // 2 for k in case.k]
        wide = _windows(d['vol'], d['origins'] - np.array(pad), G.FLIPS[0], [p + 2 * q for p, q in zip(case.dims, pad)])
        assert not _differs(y16, _conv64(_windows(d['vol'], d['origins'], G.FLIPS[0], case.dims), d['w'], d['bias'], pad))
        assert _differs(y16, _conv64(wide, d['w'], d['bias'], 0))


def test_mutant_item_0s_scale_and_shift_used_for_every_item():
    for cid in ('fstem-row-96-72', 'fstem-thin-1', 'ftconv-row-64', 'ftconv-thin-8-c16'):
        case = G.BY_ID[cid]
        d, _, y16 = G.fused_reference(cid, 'readout', case.flips[0])
        if case.kind == 'fstem':
            sc_h, sh_h, _, _ = R.stage_params(d['stem'], d['norm'])
            assert not np.array_equal(sc_h[0], sc_h[1])
            a = R.act16(R.fma16(d['stem'], sc_h[:1][EX], sh_h[:1][EX]), d['slope'])
        else:
            sc_h, sh_h, _, _ = R.stage_params(d['low'], d['lnorm'])
            low = R.act16(R.fma16(d['low'].astype(np.float64), sc_h[:1][EX], sh_h[:1][EX]), d['lslope'])
            a = np.concatenate((R.tconv_exact(low, d['tw'], d['tbias'], case.tstride)[1], R.stage16(d['skip'], d['snorm'], d['sslope'])[0]), 1)
        assert _differs(y16, G.fused_expected(case, d, a)) and not _differs(y16[:1], G.fused_expected(case, d, a)[:1])


def _off_by_one(d, flips, dims):
    """the mirrored windows one voxel off along the flipped axes (the patch's own voxels, rotated: no sentinel comes in)"""
    x = _windows(d['vol'], d['origins'], flips, dims)
    return np.roll(x, [int(f) for f in flips], (2, 3, 4))


def test_mutant_flip_off_by_one_voxel():
    for cid in ('stem1-1-3', 'stem-c4-333', 'stem-row-96-72'):
        case = G.BY_ID[cid]
        for flips in G.FLIPS[1:]:
            d, y16 = G.stem_reference(cid, 'ident', flips)
            assert _differs(y16, R.conv_exact(_off_by_one(d, flips, case.dims), d['w'], d['bias'], case.k, G.S1)[1])
            assert _differs(y16, R.stem_batch(d['vol'], d['origins'], G.FLIPS[0], case.dims, d['w'], d['bias']))
            assert not _differs(y16, R.conv_exact(_windows(d['vol'], d['origins'], flips, case.dims), d['w'], d['bias'], case.k, G.S1)[1])
    for cid in ('fstem-thin-1', 'fstem-row-96-72'):
        case = G.BY_ID[cid]
        for flips in G.FLIPS[1:]:
            d, _, y16 = G.fused_reference(cid, 'readout', flips)
            stem = R.conv_exact(_off_by_one(d, flips, case.dims), d['sw'], d['sbias'], case.k, G.S1)[1]
            assert _differs(y16, G.fused_expected(case, d, R.stage16(stem, d['norm'], d['slope'])[0]))


def test_mutant_masked_voxels_of_a_ragged_tile_counted_in_the_stems_statistics():
    case = G.BY_ID['stem1-1-3']
    d, y16 = G.stem_reference(case.id, 'stats', G.FLIPS[0])
    full = [-(-p // t) * t for p, t in zip(case.dims, (16, 8, 8))]
    x = _windows(d['vol'], d['origins'], G.FLIPS[0], case.dims)
    grown = np.pad(x, ((0, 0), (0, 0)) + tuple((0, f - p) for f, p in zip(full, case.dims)))       # zeros where the tile leaves the patch
    y_full = R.conv_exact(grown, d['w'], d['bias'], case.k, G.S1)[1]
    assert np.array_equal(y_full[(slice(None), slice(None)) + tuple(slice(0, p) for p in case.dims)], y16)
    assert not np.array_equal(R.stats_exact(y_full), R.stats_exact(y16))
    case = G.BY_ID['fstem-thin-1']                                 # ... and the norm a fused consumer applies changes with them
    d, _, y16 = G.fused_reference(case.id, 'readout', G.FLIPS[0])
    full = [-(-p // t) * t for p, t in zip(case.dims, (16, 8, 8))]
    x = _windows(d['vol'], d['origins'], G.FLIPS[0], case.dims)
    grown = np.pad(x, ((0, 0), (0, 0)) + tuple((0, f - p) for f, p in zip(full, case.dims)))
    s_full = R.conv_exact(grown, d['sw'], d['sbias'], case.k, G.S1)[1]
    sc, sh, _, _ = B.scale_shift(s_full, d['norm'][0], d['norm'][1])
    scale = s_full[0, 0].size / d['stem'][0, 0].size               # the count stays the patch's: only the sums grow
    s1, s2 = R.stats_exact(s_full)[..., 0], R.stats_exact(s_full)[..., 1]
    inv = float(np.float32(1) / np.float32(d['stem'][0, 0].size))
    mean = s1 * inv
    rstd = 1 / np.sqrt(np.maximum(s2 * inv - mean * mean, 0) + float(np.float32(1e-5)))
    sc = d['norm'][0].astype(np.float64) * rstd
    sh = d['norm'][1].astype(np.float64) - mean * sc
    assert scale > 1
    a = R.act16(R.fma16(d['stem'], B.h16(sc)[EX], B.h16(sh)[EX]), d['slope'])
    assert _differs(y16, G.fused_expected(case, d, a))


def test_mutant_x_truncated_instead_of_rounded_to_fp16():
    case = G.BY_ID['stem-row-64-8']
    d, y16 = G.stem_reference(case.id, 'round', G.FLIPS[0])
    x = _windows(d['vol'], d['origins'], G.FLIPS[0], case.dims)
    h = B.h16(x)
    trunc = np.where(np.abs(h) > np.abs(x), np.nextafter(h.astype(np.float16), np.float16(0)).astype(np.float64), h)
    assert _differs(y16, R.conv_exact(trunc, d['w'], None, case.k, G.S1)[1])
    assert not _differs(y16, R.conv_exact(h, d['w'], None, case.k, G.S1)[1])


def test_mutant_up_and_skip_chunks_swapped():
    for cid in ('ftconv-thin-4-c32', 'ftconv-row-128'):
        case = G.BY_ID[cid]
        for mode in ('ident', 'readout'):
            d, _, y16 = G.fused_reference(cid, mode, G.FLIPS[0])
            a = G.fused_staged(case, d)[0]
            assert _differs(y16, G.fused_expected(case, d, np.concatenate((a[:, 16:], a[:, :16]), 1)))


def test_mutant_one_stride_phases_tap_given_to_another():
    for cid in ('ftconv-thin-4-c16', 'ftconv-thin-8-c32', 'ftconv-row-192'):
        case = G.BY_ID[cid]
        d, _, y16 = G.fused_reference(cid, 'ident', G.FLIPS[0])
        taps = int(np.prod(case.tstride))
        for t0, t1 in ((0, 1), (taps - 2, taps - 1), (0, taps - 1)):
            tw = d['tw'].reshape(case.c, 16, taps).copy()
            tw[:, :, [t0, t1]] = tw[:, :, [t1, t0]]
            m = dict(d, tw=tw.reshape(d['tw'].shape))
            assert _differs(y16, G.fused_expected(case, m))
