"""The f16 conv and transposed-conv kernels pinned BIT FOR BIT on data on which their arithmetic is exact (tests/conv_ref.py).

Every comparison here is np.array_equal on fp16 bit patterns (zeros as +0) or on integer statistics; no tolerance.  Every
case asserts the kernel variant that ran (fnn_op_last_kernels).  The case tables and their data generators are plain Python
(no device code at import): tests/test_conv_ref_cpu.py imports them and proves, without a GPU, that every committed case is
unambiguous (stage16), exact (fits_exact, stats_fit_exact) and discriminating (mutants of the reference change it).

  (a) STAGE_CASES   the normalise-on-load arithmetic read out through a one-hot centre tap: y == stage16(x); the two kernels
                    that normalise with the fp32 rows (FP32_STAGING) against stage32's bracket
  (b) DENSE_CASES   dense integer layers, one per kernel form: identity input, crafted norm-on-load, two normalised sources
  (c) STORE_CASES   the fp16 store on ties, beyond 2048, in the subnormal range, on exact cancellation; integer statistics
  (d) CONST_CASES   constant and near-constant channels through norm-on-load

Shapes are the smallest the launch rules admit (csrc: conv_choose and the families' *_choose); where no knob lowers a
rule the batch is what reaches the rule's workgroup count on small, ragged items (noted per block below)."""
import collections
import zlib

import numpy as np
import pytest

import conv_ref as R

pytestmark = pytest.mark.gpu

Case = collections.namedtuple('Case', 'id kind n cin cin2 cout dims k stride kernel knobs modes stats')
ZR, CM = {'FNN_ZR_MIN_WGS': '1'}, {'FNN_OP_CHUNK_MAJOR': '1'}
K3, K133, K1, S1 = (3, 3, 3), (1, 3, 3), (1, 1, 1), (1, 1, 1)


def _c(id, n, cin, cin2, cout, dims, k, stride, kernel, knobs=None, modes=None, stats=True):
    modes = modes or ((('ident', 'two') if cin2 else ('ident', 'norm')) + (('stats',) if stats else ()))
    return Case(id, 'conv', n, cin, cin2, cout, tuple(dims), tuple(k), tuple(stride), kernel, dict(knobs or {}), tuple(modes), stats)


def _t(id, n, cin, cout, dims, stride, kernel, knobs=None, lds_w=False, row_store=False):
    # lds_w / row_store: what launch_tconv's rule gives the shape (asserted from the rule in the CPU test)
    return Case(id, 'tconv', n, cin, 0, cout, tuple(dims), tuple(stride), tuple(stride), kernel, dict(knobs or {}),
                ('ident', 'norm'), False), (lds_w, row_store)


GEN = 'conv3d_mfma_kernel<%d> (generic fallback)'
V1 = {'FNN_CONV_V1': '1'}
DENSE_CASES = [
    # ---- the generic kernel (FNN_CONV_V1): ragged 4 x 8 x 8 tiles, channel padding 24 -> 32
    _c('generic-1', 2, 24, 0, 16, (7, 9, 20), K3, S1, GEN % 1, V1),
    _c('generic-2', 2, 24, 0, 32, (7, 9, 20), K3, S1, GEN % 2, V1),
    _c('generic-4-cm', 2, 24, 0, 64, (7, 9, 20), K3, S1, GEN % 4, {**V1, **CM}),
    _c('generic-133-s122', 2, 24, 0, 32, (5, 12, 18), K133, (1, 2, 2), GEN % 2, V1),
    _c('generic-111', 2, 24, 0, 16, (3, 8, 9), K1, S1, GEN % 1, V1),
    # ---- conv3d_lds_kernel<nb, mb, pf>: the default of small layers, stride 1 and strided
    _c('lds-s211', 2, 32, 0, 48, (10, 6, 6), K3, (2, 1, 1), 'conv3d_lds_kernel<1,2,8>'),
    _c('lds-133-s122', 1, 16, 0, 32, (8, 12, 12), K133, (1, 2, 2), 'conv3d_lds_kernel<2,2,8>', {'FNN_NO_ZP': '1'}),
    _c('lds-313', 3, 48, 0, 80, (4, 6, 6), (3, 1, 3), S1, 'conv3d_lds_kernel<1,4,8>'),
    _c('lds-pad-8-24', 2, 8, 0, 24, (7, 9, 11), K3, S1, 'conv3d_lds_kernel<1,4,8>'),
    _c('lds-pad-40-48-cm', 2, 40, 0, 48, (7, 9, 11), K3, S1, 'conv3d_lds_kernel<1,4,8>', CM),
    _c('lds-two-src', 2, 8, 8, 16, (7, 9, 11), K3, S1, 'conv3d_lds_kernel<1,4,8>'),
    _c('lds-s222', 2, 16, 0, 32, (7, 9, 11), K3, (2, 2, 2), 'conv3d_lds_kernel<2,2,16>'),
    # ---- conv3d_persist_kernel: no knob lowers the 2048-tile rule; 72 items of 9 x 17 x 33 (2 x 3 x 5 ragged tiles) reach it.
    # Every persistent form here (these, zsp, s2) has fewer items than workgroups (PERSISTENT_WGS, asserted in the CPU test),
    # so a workgroup's tile range is shorter than an item and range seams fall INSIDE items, not only on item boundaries
    _c('persist-9tap', 72, 16, 0, 16, (9, 17, 33), K133, S1, 'conv3d_persist_kernel<1,4,1,5,1,4,0>'),
    _c('persist-9tap-two-src', 72, 16, 16, 16, (9, 17, 33), K133, S1, 'conv3d_persist_kernel<1,4,1,5,2,4,0>'),
    _c('persist-9tap-3chunks-cm', 72, 48, 0, 16, (9, 17, 33), K133, S1, 'conv3d_persist_kernel<1,8,1,5,0,8,0>', CM),
    _c('persist-111', 72, 16, 0, 16, (9, 17, 33), K1, S1, 'conv3d_persist_kernel<1,8,1,0,0,8,0>'),
    _c('persist-travelling', 72, 64, 0, 16, (9, 17, 33), K133, S1, 'conv3d_persist_kernel<1,8,0,5,0,8,0>'),   # weights too large to stay resident
    _c('persist-27-linear', 72, 16, 0, 16, (9, 17, 33), K3, S1, 'conv3d_persist_kernel<1,8,0,14,0,8,0>',
       {'FNN_ZR_MIN_WGS': '1000000000'}),                                   # (the depth-shift family refuses: the linear tap order)
    _c('persist-s222', 256, 8, 0, 24, (13, 17, 17), K3, (2, 2, 2), 'conv3d_persist_kernel<2,2,1,0,1,12,1>'),   # 4096 tiles of 2 x 8 x 8
    # ---- conv3d_zr_kernel<1 | 2, 4 | 8> (FNN_ZR_MIN_WGS=1): padded order (one chunk, FNN_NO_ZRP) and FNN_PACK_ZRP on 2, 3, 5 chunks
    _c('zr-1-8', 2, 16, 0, 16, (19, 13, 11), K3, S1, 'conv3d_zr_kernel<1,8>', ZR),
    _c('zr-1-4', 2, 16, 0, 16, (7, 13, 11), K3, S1, 'conv3d_zr_kernel<1,4>', ZR),
    _c('zr-2-8-zrp', 2, 32, 0, 32, (19, 13, 17), K3, S1, 'conv3d_zr_kernel<2,8>', ZR),
    _c('zr-2-8-padded', 2, 32, 0, 32, (19, 13, 17), K3, S1, 'conv3d_zr_kernel<2,8>', {**ZR, 'FNN_NO_ZRP': '1'}),
    _c('zr-2-8-zrp-3chunks', 2, 40, 0, 24, (19, 13, 11), K3, S1, 'conv3d_zr_kernel<2,8>', ZR),
    _c('zr-2-4-zrp-5chunks-cm', 2, 80, 0, 32, (7, 13, 17), K3, S1, 'conv3d_zr_kernel<2,4>', {**ZR, **CM}),
    _c('zr-1-4-zrp-5chunks', 2, 80, 0, 48, (7, 13, 11), K3, S1, 'conv3d_zr_kernel<1,4>', ZR),
    _c('zr-2-8-two-src', 2, 16, 32, 32, (19, 13, 17), K3, S1, 'conv3d_zr_kernel<2,8>', ZR),
    # ---- conv3d_zrw_kernel<1 | 2>: several segments, ragged last tile
    _c('zrw-1', 1, 8, 0, 16, (37, 9, 10), K3, S1, 'conv3d_zrw_kernel<1>', ZR),
    _c('zrw-2-cm', 1, 16, 0, 32, (37, 9, 17), K3, S1, 'conv3d_zrw_kernel<2>', {**ZR, **CM}),      # (one chunk in: the OUTPUT is chunk-major)
    _c('zrw-1-3segs', 2, 8, 0, 16, (69, 9, 10), K3, S1, 'conv3d_zrw_kernel<1>', ZR),
    # ---- whole-plane tiles
    _c('zr12', 2, 32, 0, 32, (17, 12, 10), K3, S1, 'conv3d_zr12_kernel<4>', ZR),
    _c('zq12-cm', 2, 32, 0, 64, (21, 11, 9), K3, S1, 'conv3d_zq12_kernel', {**ZR, **CM}),
    _c('zr12-no-zq12', 2, 32, 0, 64, (21, 11, 9), K3, S1, 'conv3d_zr12_kernel<4>', {**ZR, 'FNN_NO_ZQ12': '1'}),
    # ---- conv3d_zr_kernel<2, 10, 6>: no knob lowers the 160-unit rule
    _c('zr6', 96, 32, 0, 64, (10, 3, 3), K3, S1, 'conv3d_zr_kernel<2,10,6>'),
    _c('zr6-two-src-cm', 40, 48, 32, 64, (20, 5, 7), K3, S1, 'conv3d_zr_kernel<2,10,6>', CM),
    _c('zr6-shape-8x8x8', 96, 32, 0, 64, (10, 3, 3), K3, S1, 'conv3d_zr_kernel<2,4>', {'FNN_NO_ZR6': '1'}),
    # ---- depth-shift strided kernels: >= 768 tiles (zs), >= 4096 tiles of one chunk (zsp, zsw); odd input sizes
    _c('zs', 24, 16, 0, 32, (17, 25, 33), K3, (1, 2, 2), 'conv3d_zs_kernel<2>'),
    _c('zs-2chunks-cm', 12, 24, 0, 64, (17, 25, 33), K3, (1, 2, 2), 'conv3d_zs_kernel<2>', CM),
    _c('zsw', 128, 16, 0, 32, (25, 25, 17), K3, (1, 2, 2), 'conv3d_zsw_kernel'),
    _c('zsp', 128, 16, 0, 32, (25, 25, 17), K3, (1, 2, 2), 'conv3d_zsp_kernel', {'FNN_NO_ZSW': '1'}),
    _c('zsw-cm', 128, 16, 0, 32, (25, 25, 17), K3, (1, 2, 2), 'conv3d_zsw_kernel', CM, modes=('norm',), stats=False),   # chunk-major output
    # ---- conv3d_s2_kernel: >= 384 units of 4 x 8 x 8 x 64 channels; 64, 96 and 160 output channels; <13, 3> on planes <= 6 x 6
    _c('s2-64', 48, 32, 0, 64, (9, 17, 17), K3, (2, 2, 2), 'conv3d_s2_kernel'),
    _c('s2-96-cm', 24, 32, 0, 96, (9, 17, 17), K3, (2, 2, 2), 'conv3d_s2_kernel', CM),
    _c('s2-160', 16, 40, 0, 160, (9, 17, 17), K3, (2, 2, 2), 'conv3d_s2_kernel'),
    _c('s2-13-3', 192, 16, 0, 64, (9, 11, 9), K3, (2, 2, 2), 'conv3d_s2_kernel<13,3>'),
    _c('s2-13-3-160', 64, 24, 0, 160, (9, 11, 9), K3, (2, 2, 2), 'conv3d_s2_kernel<13,3>'),
    # ---- row kernels (the plane kernels take 16 -> 16 layers below 4 planes).  No chunk-major case: they take tensors of 16
    # channels only, which the chunk-major layout leaves as they are
    _c('row-64', 1, 16, 0, 16, (4, 8, 64), K133, S1, 'conv_row_kernel<4,1,0>'),
    _c('row-96-two-src', 2, 16, 16, 16, (4, 48, 96), K133, S1, 'conv_row_kernel<6,2,0>'),
    _c('row-160', 1, 16, 0, 16, (4, 12, 160), K133, S1, 'conv_row_kernel<10,1,0>'),
    _c('row-192-two-src', 1, 16, 16, 16, (4, 16, 192), K133, S1, 'conv_row_kernel<12,2,0>'),
    # more (plane, strip) units than the persistent grid (ROW_OVER_GRID): a workgroup walks from unit to unit, across planes and
    # - 7 x 86 = 602 units is the smallest such count - across an item boundary (CPU test)
    _c('row-64-over-grid', 7, 16, 0, 16, (86, 8, 64), K133, S1, 'conv_row_kernel<4,1,0>'),
    _c('row-64-two-src-over-grid', 7, 16, 16, 16, (86, 8, 64), K133, S1, 'conv_row_kernel<4,2,0>'),
    # ---- plane kernels (conv2d_zp.hip), stride 1 and (1, 2, 2), half image and FNN_ZP_NO_HALF / FNN_ZPS_NO_HALF
    _c('zp-8-4', 2, 32, 0, 32, (1, 19, 70), K133, S1, 'conv2d_zp_kernel<8,4>'),
    _c('zp-8-2-two-src-cm', 2, 48, 16, 32, (3, 21, 30), K133, S1, 'conv2d_zp_kernel<8,2>', CM),
    _c('zp-4-1', 2, 96, 0, 96, (1, 13, 14), K133, S1, 'conv2d_zp_kernel<4,1>'),
    _c('zp-half', 2, 16, 0, 32, (2, 33, 70), K133, S1, 'conv2d_zp_kernel<8,4,2,half>'),
    _c('zp-no-half', 2, 16, 0, 32, (2, 33, 70), K133, S1, 'conv2d_zp_kernel<8,4>', {'FNN_ZP_NO_HALF': '1'}),
    _c('zp-half-two-src-1blk', 2, 16, 16, 16, (1, 37, 83), K133, S1, 'conv2d_zp_kernel<8,4,1,half>'),
    _c('zp-1blk', 2, 32, 0, 16, (1, 19, 40), K133, S1, 'conv2d_zp_kernel<8,4,1>'),
    _c('zps-4-2', 2, 32, 0, 64, (1, 37, 45), K133, (1, 2, 2), 'conv2d_zps_kernel<4,2>'),
    _c('zps-2-2-two-src', 2, 48, 16, 96, (2, 30, 44), K133, (1, 2, 2), 'conv2d_zps_kernel<2,2>'),
    _c('zps-half', 2, 16, 0, 32, (3, 21, 38), K133, (1, 2, 2), 'conv2d_zps_kernel<2,2,half>'),
    _c('zps-no-half', 2, 16, 0, 32, (3, 21, 38), K133, (1, 2, 2), 'conv2d_zps_kernel<2,2>', {'FNN_ZPS_NO_HALF': '1'}),
    _c('zps-4-1', 2, 96, 0, 64, (1, 9, 7), K133, (1, 2, 2), 'conv2d_zps_kernel<4,1>'),
]
# tconv_mfma_kernel<NBT, TG>: each with the weights through LDS (>= 4 k-steps: more than 96 input channels) off and on and
# whole-row stores (w stride 2, two cout blocks: NBT = 2 only) off and on - every combination launch_tconv can reach; voxel
# counts that are no multiple of 256.  lds_w / row_store are not observable through the C ABI: the flags below restate
# launch_tconv's rule (tconv.hip) and the CPU test checks the cases against that restatement - if the rule changes, both
# must be changed together
TCONV = [
    _t('tconv-1-4', 1, 21, 10, (3, 4, 5), (2, 2, 2), 'tconv_mfma_kernel<1,4>'),
    _t('tconv-1-4-ldsw', 1, 136, 16, (3, 4, 5), (2, 2, 2), 'tconv_mfma_kernel<1,4>', lds_w=True),
    _t('tconv-2-2-ldsw-cm', 2, 160, 160, (5, 3, 3), (2, 1, 1), 'tconv_mfma_kernel<2,2>', CM, lds_w=True),
    _t('tconv-2-2-no-ldsw', 2, 160, 160, (5, 3, 3), (2, 1, 1), 'tconv_mfma_kernel<2,2>', {'FNN_TCONV_NO_LDSW': '1'}),
    _t('tconv-1-2', 2, 40, 48, (5, 3, 7), (2, 1, 1), 'tconv_mfma_kernel<1,2>'),
    _t('tconv-1-2-ldsw', 2, 136, 48, (5, 3, 7), (2, 1, 1), 'tconv_mfma_kernel<1,2>', lds_w=True),
    _t('tconv-2-2-rowstore', 1, 64, 32, (4, 6, 6), (1, 1, 2), 'tconv_mfma_kernel<2,2>', row_store=True),
    _t('tconv-2-2-ldsw-rowstore', 1, 128, 32, (3, 5, 7), (1, 1, 2), 'tconv_mfma_kernel<2,2>', lds_w=True, row_store=True),
    _t('tconv-2-4-ldsw-no-rowstore', 1, 128, 32, (3, 5, 7), (2, 2, 1), 'tconv_mfma_kernel<2,4>', lds_w=True),
    _t('tconv-2-4-rowstore', 1, 64, 32, (4, 6, 6), (1, 2, 2), 'tconv_mfma_kernel<2,4>', row_store=True),
    _t('tconv-2-4-no-rowstore', 1, 64, 32, (4, 6, 6), (1, 2, 2), 'tconv_mfma_kernel<2,4>', {'FNN_TCONV_NO_ROWSTORE': '1'}),
    _t('tconv-2-4-ldsw-rowstore', 1, 128, 32, (3, 5, 7), (2, 2, 2), 'tconv_mfma_kernel<2,4>', lds_w=True, row_store=True),
    _t('tconv-2-4-257-voxels', 1, 32, 64, (1, 1, 257), (2, 2, 2), 'tconv_mfma_kernel<2,4>', row_store=True),
]
# the statistics are sums of the ROUNDED outputs, not of the fp32 accumulators: odd integers beyond 2048 round to even ones in
# the store; a dozen voxels per (item, channel) keep the sums of squares exact (stats_fit_exact, in units of the quantum 2)
DENSE_CASES += [
    _c('stats-rounded-lds', 2, 16, 0, 16, (2, 2, 3), K1, S1, 'conv3d_lds_kernel<1,4,8>', modes=('statsround',)),
    _c('stats-rounded-zr', 2, 16, 0, 16, (4, 1, 3), K3, S1, 'conv3d_zr_kernel<1,4>', ZR, modes=('statsround',)),
    _c('stats-rounded-zp', 2, 32, 0, 32, (1, 3, 4), K133, S1, 'conv2d_zp_kernel<4,1>', modes=('statsround',)),
]
TCONV_FLAGS = {c.id: f for c, f in TCONV}
DENSE_CASES += [c for c, _ in TCONV]
BY_ID = {c.id: c for c in DENSE_CASES}
assert len(BY_ID) == len(DENSE_CASES)

# every kernel form the issue names; each appears as some case's asserted kernel (the closing test)
REQUIRED_KERNELS = {
    GEN % 1, GEN % 2, GEN % 4, 'conv3d_lds_kernel<1,2,8>', 'conv3d_lds_kernel<2,2,8>', 'conv3d_lds_kernel<1,4,8>',
    'conv3d_lds_kernel<2,2,16>', 'conv3d_persist_kernel<1,4,1,5,1,4,0>', 'conv3d_persist_kernel<1,4,1,5,2,4,0>',
    'conv3d_persist_kernel<1,8,1,5,0,8,0>', 'conv3d_persist_kernel<1,8,1,0,0,8,0>', 'conv3d_persist_kernel<1,8,0,5,0,8,0>',
    'conv3d_persist_kernel<1,8,0,14,0,8,0>', 'conv3d_persist_kernel<2,2,1,0,1,12,1>',
    'conv3d_zr_kernel<1,8>', 'conv3d_zr_kernel<1,4>', 'conv3d_zr_kernel<2,8>', 'conv3d_zr_kernel<2,4>', 'conv3d_zrw_kernel<1>',
    'conv3d_zrw_kernel<2>', 'conv3d_zr12_kernel<4>', 'conv3d_zq12_kernel', 'conv3d_zr_kernel<2,10,6>', 'conv3d_zs_kernel<2>',
    'conv3d_zsp_kernel', 'conv3d_zsw_kernel', 'conv3d_s2_kernel', 'conv3d_s2_kernel<13,3>', 'conv_row_kernel<4,1,0>',
    'conv_row_kernel<4,2,0>', 'conv_row_kernel<6,2,0>', 'conv_row_kernel<10,1,0>', 'conv_row_kernel<12,2,0>', 'conv2d_zp_kernel<8,4>', 'conv2d_zp_kernel<8,2>',
    'conv2d_zp_kernel<4,1>', 'conv2d_zp_kernel<8,4,2,half>', 'conv2d_zp_kernel<8,4,1,half>', 'conv2d_zp_kernel<8,4,1>',
    'conv2d_zps_kernel<4,2>', 'conv2d_zps_kernel<2,2>', 'conv2d_zps_kernel<2,2,half>', 'conv2d_zps_kernel<4,1>',
    'tconv_mfma_kernel<1,2>', 'tconv_mfma_kernel<1,4>', 'tconv_mfma_kernel<2,2>', 'tconv_mfma_kernel<2,4>',
}

# (c): the store on chosen magnitudes, through every family's epilogue (the persistent, stride-2, six-row, whole-plane and
# walking kernels have epilogue code of their own); the transposed conv with and without whole-row stores
STORE_CASES = ['generic-2', 'lds-pad-8-24', 'lds-s222', 'persist-9tap', 'persist-9tap-3chunks-cm', 'persist-27-linear', 'persist-s222',
               'zr-1-8', 'zr-2-8-zrp', 'zrw-2-cm', 'zr12', 'zq12-cm', 'zr6', 'zs', 'zsw', 'zsp', 's2-64', 's2-13-3', 'row-96-two-src',
               'zp-8-4', 'zps-half', 'tconv-1-4', 'tconv-1-2-ldsw', 'tconv-2-2-rowstore', 'tconv-2-4-rowstore', 'tconv-2-4-no-rowstore']
# workgroups of the persistent forms' grids (conv3d.hip: 256 CUs x wpc >= 2, or c.gx = 512; conv3d_zr.hip zsp: 512;
# conv3d_s2.hip: 256): more than any such case's items
PERSISTENT_WGS = {'conv3d_persist_kernel': 512, 'conv3d_zsp_kernel': 512, 'conv3d_s2_kernel': 256}
# the row kernels' grid (conv3d_row.hip launch_row_t: 256 CUs x min(what LDS admits, cap); W = 64: cap = 2 for one chunk
# (25856 B: six fit) and for two (51200 B: three fit)): fewer than these cases' units
ROW_OVER_GRID = {'row-64-over-grid': 512, 'row-64-two-src-over-grid': 512}
STORE_MODES = ('ties', 'subnormal')
# (d): constant / near-constant channels through norm-on-load: three channels (padded to 16: the shift must not reach the
# padding), (1, 3, 3) taps of +-1 - few enough products that the sums of these arbitrary fp16 values stay exact (CPU test)
CONST_CASES = [
    _c('const-lds', 2, 3, 0, 16, (6, 12, 20), K133, S1, 'conv3d_lds_kernel<1,4,8>', modes=('const',), stats=False),
    _c('const-zp', 2, 3, 0, 32, (1, 19, 70), K133, S1, 'conv2d_zp_kernel<8,4,2,half>', modes=('const',), stats=False),
    _c('const-row', 2, 3, 0, 16, (4, 8, 64), K133, S1, 'conv_row_kernel<4,1,0>', modes=('const',), stats=False),
]
# per source: targets of craft_norm (offset into R.F16_TARGETS per channel) and the dyadic slope
SRC_NORM = ((0, 0.25), (2, 0.5))


def _seed(*what):
    return zlib.crc32(repr(what).encode()) % (2 ** 31)


def _permuted_items(first, n):
    """[c, voxels] -> [n, c, voxels]: every item holds item 0's values of each channel at other positions (a rotation)"""
    return np.stack([np.roll(first, 13 * i + (i > 0), axis=1) for i in range(n)])


def case_data(case, mode):
    """The operands of a dense exact layer -> dict(x, x2, norm, slope, norm2, slope2, w, bias); float32 arrays.
    ident: integers in [-3, 3], no norm.  norm / two: even integers in [-8, 8] per source with craft_norm's (gamma, beta) for
    fp16-exact (S, H) per channel and a dyadic slope - the staged values stay dyadic; `two` gives the second source OTHER
    (S, H, slope).  ties: multiples of 16 (of 64 for a transposed conv, whose outputs sum over the channels of ONE tap) and
    biases of +-0.5 / 0 (outputs k + 0.5 in the binades of spacing 1, beyond 2048, exact zeros).  statsround: as stats with
    integer biases of 2111 .. 2200 - odd outputs beyond 2048, which the store rounds to even.  subnormal: operands of quantum 2^-12 and 2^-14, outputs in fp16's subnormal range.  const: see const_data.
    Weights: dense integers of {-2, -1, 1, 2}; bias: odd multiples of 0.25.  stats: activations of {-1, 0, 1}, weights of
    +-1, odd integer biases - outputs small enough that their sums of squares stay below 2^24 (stats_fit_exact)."""
    if mode == 'const':
        return const_data(case)
    rs = np.random.RandomState(_seed(case.id, mode))
    vox = int(np.prod(case.dims))
    d = dict(x2=None, norm=None, slope=1.0, norm2=None, slope2=1.0)
    srcs = []
    for i, c in enumerate((case.cin, case.cin2)):
        if not c:
            continue
        if mode in ('norm', 'two'):
            first = 2.0 * rs.randint(-4, 5, (c, vox))
            x = _permuted_items(first, case.n).reshape(case.n, c, *case.dims)
            off, slope = SRC_NORM[i]
            S = np.array([R.F16_TARGETS[(ch + off) % 4][0] for ch in range(c)])
            H = np.array([R.F16_TARGETS[(ch + off) % 4][1] for ch in range(c)])
            srcs.append((x.astype(np.float32), R.craft_norm(x, S, H), slope))
        else:
            x = (rs.randint(-1, 2, (case.n, c, *case.dims)) if mode in ('stats', 'statsround') else rs.randint(-3, 4, (case.n, c, *case.dims))).astype(np.float64)
            x = x * {'ties': 64.0 if case.kind == 'tconv' else 16.0, 'subnormal': 2.0 ** -12}.get(mode, 1.0)
            srcs.append((x.astype(np.float32), None, 1.0))
    d['x'], d['norm'], d['slope'] = srcs[0]
    if case.cin2:
        d['x2'], d['norm2'], d['slope2'] = srcs[1]
    ctot = case.cin + case.cin2
    shape = (ctot, case.cout, *case.k) if case.kind == 'tconv' else (case.cout, ctot, *case.k)
    w = rs.choice([-2.0, -1.0, 1.0, 2.0], shape)
    bias = (2 * rs.randint(-4, 4, case.cout) + 1) * 0.25
    if mode == 'ties':
        bias = np.array([0.5, 0.0, -0.5])[np.arange(case.cout) % 3]
    if mode == 'stats':
        w, bias = np.sign(w), 2.0 * rs.randint(-2, 2, case.cout) + 1
    if mode == 'statsround':
        w, bias = np.sign(w), 2111.0 + rs.randint(0, 90, case.cout)
    if mode == 'subnormal':
        w = w * 2.0 ** -14
        bias = np.where(np.arange(case.cout) % 2 == 0, 0.0, (2 * rs.randint(-4, 4, case.cout) + 1) * 2.0 ** -26)
    d['w'], d['bias'] = w.astype(np.float32), bias.astype(np.float32)
    return d


def const_data(case):
    """(d): channel 0 one value everywhere (var = 0: rstd = 1 / sqrt(eps)), channel 1 the same with one voxel different,
    channel 2 with mean / std about 1e3 (values 999.5, 1000, 1000.5); ordinary gamma and beta, a dyadic slope; weights of
    +-1, no bias."""
    rs = np.random.RandomState(_seed(case.id, 'const'))
    assert case.cin == 3
    x = np.empty((case.n, case.cin, *case.dims))
    x[:, 0] = 3.0
    x[:, 1] = -2.0
    x[:, 1, 0, 1, 2] = -1.5
    x[:, 2] = 1000.0 + 0.5 * rs.randint(-1, 2, (case.n, *case.dims))
    gamma = (rs.rand(case.cin) * 0.5 + 0.75).astype(np.float32)
    beta = (rs.randn(case.cin) * 0.5 + np.array([1.0, -1.0, 0.25])).astype(np.float32)
    gamma[0] = np.float32(2.0 ** -9)              # rstd = 316: the scale is 0.6, the shift beta - 3 * 0.6
    w = rs.choice([-1.0, 1.0], (case.cout, case.cin, *case.k))
    return dict(x=x.astype(np.float32), x2=None, norm=(gamma, beta), slope=0.25, norm2=None, slope2=1.0, w=w.astype(np.float32),
                bias=None)


def case_staged(d, margin=1.0):
    """the staged activations of both sources, concatenated -> (value, lo, hi, ambiguous)"""
    parts = [R.stage16(d['x'], d['norm'], d['slope'], margin=margin)]
    if d['x2'] is not None:
        parts.append(R.stage16(d['x2'], d['norm2'], d['slope2'], margin=margin))
    return tuple(np.concatenate([p[i] for p in parts], 1) for i in range(3)) + (sum(p[3] for p in parts),)


def case_reference(case, d, a=None):
    """(t, y16) of the case on the staged activations a (default: case_staged's value)"""
    a = case_staged(d)[0] if a is None else a
    if case.kind == 'tconv':
        return R.tconv_exact(a, d['w'], d['bias'], case.stride, fast=True)
    return R.conv_exact(a, d['w'], d['bias'], case.k, case.stride, fast=True)


# ---- (a) --------------------------------------------------------------------------------------------------------------
# id, kind, cin, cout, dims, k, stride, kernel, knobs.  20480 voxels per channel = the sweep once; 32 channels wherever the
# kernel takes them, so that FNN_OP_CHUNK_MAJOR changes the layout (it leaves tensors of 16 channels alone)
Stage = collections.namedtuple('Stage', 'id kind cin cout dims k stride kernel knobs')
STAGE_CASES = [
    Stage('generic', 'conv', 32, 32, (8, 40, 64), K3, S1, GEN % 2, V1),
    Stage('lds', 'conv', 32, 32, (8, 40, 64), K3, S1, 'conv3d_lds_kernel<1,4,8>', {}),
    Stage('zr-1-8', 'conv', 32, 16, (8, 40, 64), K3, S1, 'conv3d_zr_kernel<1,8>', ZR),
    Stage('zr-2-4', 'conv', 32, 32, (4, 80, 64), K3, S1, 'conv3d_zr_kernel<2,4>', ZR),
    Stage('zrw', 'conv', 16, 16, (32, 20, 32), K3, S1, 'conv3d_zrw_kernel<1>', ZR),
    Stage('row', 'conv', 16, 16, (5, 64, 64), K133, S1, 'conv_row_kernel<4,1,0>', {}),
    Stage('plane', 'conv', 32, 32, (1, 160, 128), K133, S1, 'conv2d_zp_kernel<8,4>', {}),
    Stage('tconv', 'tconv', 32, 32, (8, 40, 64), (1, 2, 2), (1, 2, 2), 'tconv_mfma_kernel<2,4>', {}),
]
STAGE_SLOPES = (0.01, 1.0, 0.0)
# the two kernels that keep the fp32 scale / shift rows and an fp32 fma (conv3d.hip; fnn_device.h says why): their staged
# value is conv_ref.stage32's bracket, one fp16 value for all but a few elements in a thousand
FP32_STAGING = ('conv3d_mfma_kernel', 'conv3d_lds_kernel')
STAGE_SALT = {'row': 1, 'plane': 1}      # other data where a draw's scale or shift sat on an fp16 rounding boundary (CPU test)


def sweep16():
    """every fp16 value, both signs, of the subnormals and the two binades above them and of the seven binades 2^-4 .. 2^3"""
    exps = [0, 1, 2] + list(range(11, 18))
    bits = np.concatenate([(e << 10) + np.arange(1024) for e in exps]).astype(np.uint16)
    return np.concatenate([bits, bits | 0x8000]).view(np.float16).astype(np.float64)


def stage_data(sc):
    """x [1, cin, *dims]: per channel the sweep in an order of its own, a channel-dependent share of it made positive (a mean
    away from 0); ordinary random gamma, beta"""
    rs = np.random.RandomState(_seed('stage', sc.id, STAGE_SALT.get(sc.id, 0)))
    vox = int(np.prod(sc.dims))
    sw = sweep16()
    x = np.empty((sc.cin, vox))
    for c in range(sc.cin):
        v = np.resize(sw[rs.permutation(sw.size)], vox)
        x[c] = np.where(np.arange(vox) % 4 < c % 4, np.abs(v), v)
    gamma = (rs.rand(sc.cin) + 0.5).astype(np.float32)
    beta = (rs.randn(sc.cin) * 0.3).astype(np.float32)
    if sc.kind == 'tconv':                            # [cin][cout][tap]: tap t of output channel co reads input channel co + t
        w = np.zeros((sc.cin, sc.cout, int(np.prod(sc.k))), np.float32)
        for co in range(sc.cout):
            for t in range(w.shape[2]):
                w[(co + t) % sc.cin, co, t] = 1.0
        w = w.reshape(sc.cin, sc.cout, *sc.k)
    else:
        w = np.zeros((sc.cout, sc.cin, *sc.k), np.float32)
        for co in range(sc.cout):
            w[(co, (co * 5 + 3) % sc.cin) + tuple(i // 2 for i in sc.k)] = 1.0
    return x.reshape(1, sc.cin, *sc.dims).astype(np.float32), gamma, beta, w


def stage_expected(sc, v):
    """what the one-hot weights of stage_data read out of the staged tensor v [1, cin, *dims]"""
    if sc.kind != 'tconv':
        return v[:, [(co * 5 + 3) % sc.cin for co in range(sc.cout)]]
    s = sc.stride
    out = np.empty((1, sc.cout, *[sc.dims[i] * s[i] for i in range(3)]))
    for co in range(sc.cout):
        for t, (a, b, c) in enumerate(np.ndindex(*s)):
            out[0, co, a::s[0], b::s[1], c::s[2]] = v[0, (co + t) % sc.cin]
    return out


# ---- device side -------------------------------------------------------------------------------------------------------
SEEN = {}                        # case id -> kernels asserted (the closing test)


def _bits(y):
    with np.errstate(over='ignore'):
        return (np.asarray(y, np.float64) + 0.0).astype(np.float16).view(np.uint16)


def _same_bits(got, want, what):
    g, w = _bits(got), _bits(want)
    if not np.array_equal(g, w):
        bad = np.argwhere(g != w)
        i = tuple(bad[0])
        raise AssertionError(f'{what}: {len(bad)} of {g.size} values differ, first at {i}: device {float(np.asarray(got)[i])!r} '
                             f'({g[i]:#06x}), reference {float(np.asarray(want)[i])!r} ({w[i]:#06x})')


def _launch(case, d, monkeypatch, want_stats=False):
    from fast_nnunet_amd import capi
    for name in ('FNN_ZR_MIN_WGS', 'FNN_CONV_V1', 'FNN_NO_ZRP', 'FNN_NO_ZR6', 'FNN_NO_ZQ12', 'FNN_NO_ZSW', 'FNN_NO_ZP', 'FNN_NO_ROW',
                 'FNN_OP_CHUNK_MAJOR', 'FNN_TCONV_NO_LDSW', 'FNN_TCONV_NO_ROWSTORE', 'FNN_ZP_NO_HALF', 'FNN_ZPS_NO_HALF', 'FNN_OP_F8'):
        monkeypatch.delenv(name, raising=False)
    for name, v in case.knobs.items():
        monkeypatch.setenv(name, v)
    g, b = d['norm'] if d['norm'] is not None else (None, None)
    if case.kind == 'tconv':
        out = capi.op_conv_transpose3d(d['x'], d['w'], d['bias'], case.stride, gamma=g, beta=b, slope=d['slope'])
        out = (out, None) if want_stats else out
    else:
        g2, b2 = d['norm2'] if d['norm2'] is not None else (None, None)
        out = capi.op_conv3d(d['x'], d['w'], d['bias'], case.k, case.stride, gamma=g, beta=b, slope=d['slope'], x2=d['x2'],
                             gamma2=g2, beta2=b2, slope2=d['slope2'], want_stats=want_stats)
    ran = capi.op_last_kernels()
    assert ran == [case.kernel], f'{case.id}: ran {ran}, the case is written for {case.kernel}'
    SEEN.setdefault(case.id, set()).update(ran)
    return out


@pytest.mark.parametrize('slope', STAGE_SLOPES)
@pytest.mark.parametrize('sc', STAGE_CASES, ids=lambda s: s.id)
def test_staging_arithmetic_read_out_through_a_one_hot_tap(sc, slope, monkeypatch):
    """(a): y == stage16(x) bit for bit over dense sweeps of fp16 values (ties of the fused multiply-add, cancellation into
    the subnormal range, slope products in the subnormal range), channels-last and chunk-major."""
    x, gamma, beta, w = stage_data(sc)
    fp32 = sc.kernel.startswith(FP32_STAGING)
    if fp32:
        _, lo, hi, n_open = R.stage32(x, (gamma, beta), slope)
        lo, hi = stage_expected(sc, lo), stage_expected(sc, hi)
        assert n_open <= 1e-2 * x.size
    else:
        v, _, _, amb = R.stage16(x, (gamma, beta), slope)
        assert amb == 0
        want = stage_expected(sc, v)
    for cm in ((False, True) if sc.cin > 16 else (False,)):
        case = Case('stage-' + sc.id, sc.kind, 1, sc.cin, 0, sc.cout, sc.dims, sc.k, sc.stride, sc.kernel,
                    {**sc.knobs, **(CM if cm else {})}, (), False)
        d = dict(x=x, x2=None, norm=(gamma, beta), slope=slope, norm2=None, slope2=1.0, w=w, bias=None)
        y = _launch(case, d, monkeypatch)
        what = f'staging through {sc.kernel}, slope {slope}, chunk-major {cm}'
        if fp32:
            out = (y < lo) | (y > hi)
            assert not out.any(), f'{what}: {int(out.sum())} of {y.size} values outside the fp32 form\'s bracket'
            _same_bits(np.where(lo == hi, y, 0.0), np.where(lo == hi, lo, 0.0), what)
        else:
            _same_bits(y, want, what)


DENSE_RUNS = [(c.id, m) for c in DENSE_CASES for m in c.modes]


@pytest.mark.parametrize('cid,mode', DENSE_RUNS, ids=lambda v: str(v))
def test_dense_exact_layer(cid, mode, monkeypatch):
    """(b): dense integer weights on every tap and channel, dyadic bias, ragged tiles, n > 1: the device EQUALS the
    float64 result rounded once; where the outputs' sums of squares stay below 2^24 quanta (mode `stats`: by construction) the
    statistics are those integers - replica atomics, per-tile slot rows, persistent chains, several workgroups per (item,
    channel), more items than replica rows."""
    case = BY_ID[cid]
    d = case_data(case, mode)
    a, _, _, amb = case_staged(d)
    assert amb == 0
    _, y16 = case_reference(case, d, a)
    y, stats = _launch(case, d, monkeypatch, want_stats=True)
    _same_bits(y, y16, f'{cid} [{mode}]')
    if case.kind == 'conv' and R.stats_fit_exact(y16):
        assert np.array_equal(stats, R.stats_exact(y16)), f'{cid} [{mode}]: statistics'
    else:
        assert mode not in ('stats', 'statsround'), f'{cid}: the case claims exact statistics'


@pytest.mark.parametrize('mode', STORE_MODES)
@pytest.mark.parametrize('cid', STORE_CASES)
def test_store_rounds_the_exact_sum_once(cid, mode, monkeypatch):
    """(c): f16(acc + bias) on ties (k + 0.5 in the binades of spacing 1), beyond 2048, on exact cancellation to 0 and in
    the subnormal range (ties of the 2^-24 grid): one round-to-nearest-even of the exact value."""
    case = BY_ID[cid]
    d = case_data(case, mode)
    _, y16 = case_reference(case, d)
    y = _launch(case, d, monkeypatch)
    _same_bits(y, y16, f'{cid} [{mode}]')


@pytest.mark.parametrize('case', CONST_CASES, ids=lambda c: c.id)
def test_constant_and_near_constant_channels_through_norm_on_load(case, monkeypatch):
    """(d): var = 0, one voxel different, mean / std about 1e3: y lies in stage16's bracket pushed through the conv - of
    width 0 (bit equality) wherever scale and shift round unambiguously, which the CPU test shows for this data."""
    d = case_data(case, 'const')
    if case.kernel.startswith(FP32_STAGING):
        a, lo, hi, amb = R.stage32(d['x'], d['norm'], d['slope'])
    else:
        a, lo, hi, amb = case_staged(d)
    t, y16 = case_reference(case, d, a)
    y = _launch(case, d, monkeypatch)
    if amb == 0:
        _same_bits(y, y16, case.id)
    else:                                                          # the |w|-weighted sum of the bracket widths; rounding is monotone
        assert R.fits_exact(lo, d['w'], None) and R.fits_exact(hi, d['w'], None)
        width, _ = R.conv_exact(hi - lo, np.abs(d['w']), None, case.k, case.stride)
        assert (y >= R.h16(t - width)).all() and (y <= R.h16(t + width)).all()
        exact = width == 0
        _same_bits(np.where(exact, y, 0.0), np.where(exact, y16, 0.0), case.id)


def test_every_named_kernel_form_is_asserted_by_a_case():
    """The closing test: every form of the issue's table is the asserted kernel of a committed case, and whatever ran in
    this session ran what its case names (after a full run of this file: all of them)."""
    named = {c.kernel for c in DENSE_CASES} | {s.kernel for s in STAGE_CASES}
    assert REQUIRED_KERNELS <= named, sorted(REQUIRED_KERNELS - named)
    ran = set().union(*SEEN.values()) if SEEN else set()
    assert ran <= named | {c.kernel for c in CONST_CASES}
    if all(c.id in SEEN for c in DENSE_CASES):
        assert REQUIRED_KERNELS <= ran, sorted(REQUIRED_KERNELS - ran)
