"""The rule of the dynamic-table deflate encoder (csrc/deflate_dyn_core.h) on its Python model (tests/deflate_dyn_ref.py),
without a GPU: zlib reads every fragment, the code lengths obey Kraft and their limits, no fragment is longer than the fixed
code's, the length limit and the choice between the two codes are both exercised, and the golden mask's fragment is no
larger than what the host writer makes at zlib level 1.  The GPU test compares the kernels with this model byte for byte."""
import gzip
import heapq
import os
import zlib
from fractions import Fraction

import numpy as np
import pytest

import deflate_dyn_ref as dyn
import deflate_ref
from test_gpu_deflate import CONTENTS, LENGTHS, MASK, _file_bytes

C = deflate_ref.CHUNK


def _kraft(lens):
    return sum(Fraction(1, 2 ** n) for n in lens if n)


def _check_chunk_tables(chunk, elem):
    lens, hlit, coded, cllens, hclen, _ = dyn.tables(dyn.chunk_symbols(chunk, elem))
    used = {s for s, _, _, _ in dyn.chunk_symbols(chunk, elem)}
    assert len(used) >= 2 and 256 in used, 'the invariant: a literal and 256'
    assert {s for s in range(dyn.NLIT) if lens[s]} == used, 'length 0 goes exactly to frequency 0'
    assert max(lens) <= 15 and _kraft(lens) == 1
    assert max(cllens) <= 7 and _kraft(cllens) == 1
    assert 257 <= hlit <= 286 and 4 <= hclen <= 19


@pytest.mark.parametrize('kind', list(CONTENTS))
def test_zlib_inflates_every_fragment_and_none_is_longer_than_the_fixed_codes(kind):
    rng = np.random.default_rng(sorted(CONTENTS).index(kind))
    for n in LENGTHS:
        if kind == 'uint16_stays_with_255' and n < 2:
            continue
        values, narrow = CONTENTS[kind](rng, n)
        raw, elem = _file_bytes(values, narrow)
        frag, dynamic_chunks = dyn.fragment(raw, elem)
        assert deflate_ref.inflate(frag) == raw, (kind, n)
        assert len(frag) <= len(deflate_ref.fragment(raw, elem)), (kind, n)
        assert 0 <= dynamic_chunks <= -(-len(raw) // C)
        for c in range(0, min(len(raw), 3 * C), C):
            _check_chunk_tables(raw[c:c + C], elem)


def _unlimited_depth(freqs):
    """The longest code of a plain Huffman code (a heap, no limit) - written here, not taken from the model.  Among nodes of
    equal weight the one made last is merged first, as in the rule; every such choice gives a code of the same cost, and
    this one is the deep one (the shallowest optimal code of Fibonacci frequencies with one more 1 is 10 deep)."""
    heap = [(f, 0, 0) for f in freqs]                             # (weight, minus the time it was made, depth)
    heapq.heapify(heap)
    made = 0
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        made += 1
        heapq.heappush(heap, (a[0] + b[0], -made, max(a[2], b[2]) + 1))
    return heap[0][2]


def test_the_length_limit_is_exercised_by_fibonacci_frequencies():
    chunk = dyn.fibonacci_chunk()
    assert len(chunk) == 10945 and len(set(chunk)) == 19 and all(a != b for a, b in zip(chunk, chunk[1:]))
    freq = sorted(chunk.count(v) for v in set(chunk))
    assert freq[:6] == [1, 1, 2, 3, 5, 8] and freq[-1] == 4181
    assert _unlimited_depth(freq + [1]) > 15, 'a plain Huffman code of this chunk is too deep for deflate'
    lens = dyn.tables(dyn.chunk_symbols(chunk, 1))[0]
    assert max(lens) == 15 and _kraft(lens) == 1
    frag, dynamic_chunks = dyn.fragment(chunk, 1)
    assert dynamic_chunks == 1 and deflate_ref.inflate(frag) == chunk


def test_the_choice_is_exercised():
    frag, dynamic_chunks = dyn.fragment(dyn.TINY_CHUNK, 1)
    assert dynamic_chunks == 0 and frag == deflate_ref.fragment(dyn.TINY_CHUNK, 1), 'a few bytes take the fixed code'
    full = (np.arange(C) // 100 % 5).astype(np.uint8).tobytes()
    frag, dynamic_chunks = dyn.fragment(full, 1)
    assert dynamic_chunks == 1 and len(frag) < len(deflate_ref.fragment(full, 1)) and deflate_ref.inflate(frag) == full
    assert frag[0] & 7 == 4, 'BFINAL 0, BTYPE 10'
    both, dynamic_chunks = dyn.fragment(full + dyn.TINY_CHUNK, 1)
    assert dynamic_chunks == 1 and both == frag + deflate_ref.fragment(dyn.TINY_CHUNK, 1), 'chunks are independent'


def test_code_lengths_and_the_run_length_rule():
    assert dyn.code_lengths([0, 5, 0, 0], 15) == [0, 1, 0, 0], 'one used symbol: length 1'
    assert dyn.code_lengths([3, 3], 15) == [1, 1]
    assert dyn.code_lengths([1, 1, 1, 1, 0], 7) == [2, 2, 2, 2, 0]
    assert dyn.code_lengths([1, 2, 4, 8], 2) == [2, 2, 2, 2], 'depths 3, 3, 2, 1 clamped to 2, then the leaf at 1 moves down'
    assert dyn.canonical([3, 3, 3, 3, 3, 2, 4, 4]) == [2, 3, 4, 5, 6, 0, 14, 15], 'the example of RFC 1951 3.2.2'
    r = dyn.run_length
    assert r([0] * 2 + [5] * 3) == [(0, 0, 0), (0, 0, 0), (5, 0, 0), (5, 0, 0), (5, 0, 0)]
    assert r([5] * 4) == [(5, 0, 0), (16, 2, 0)] and r([5] * 8) == [(5, 0, 0), (16, 2, 3), (5, 0, 0)]
    assert r([0] * 3) == [(17, 3, 0)] and r([0] * 10) == [(17, 3, 7)] and r([0] * 11) == [(18, 7, 0)]
    assert r([0] * 139) == [(18, 7, 127), (0, 0, 0)]
    assert r([7, 1, 1, 1, 1]) == [(7, 0, 0), (1, 0, 0), (16, 2, 0)], 'a run crosses into the distance lengths'


def test_the_library_exports_the_entry_point_in_abi_4():
    import re
    from fast_nnunet_amd import capi
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = re.sub(r'/\*.*?\*/', '', open(os.path.join(root, 'include', 'fnn.h')).read(), flags=re.S)
    lib = capi.load_library()
    assert re.search(r'\bfnn_deflate_labels_dyn\s*\(', header) and 'fnn_deflate_labels_dyn' in capi.EXPORTS and hasattr(lib, 'fnn_deflate_labels_dyn')
    assert lib.fnn_abi_version() == 4


def test_the_switch_takes_three_values_and_the_mask_encoder_two(tmp_path):
    """Constructing a predictor touches no GPU.  False and True stay what they were; 'dynamic' is kept as it is; anything else
    is refused at construction, and by the folder functions before a file is read."""
    from fast_nnunet_amd import nnUNetPredictor
    from fast_nnunet_amd import postprocessing as pp
    from fast_nnunet_amd.case_pipeline import compress_mode, device_compressor
    from fast_nnunet_amd.imageio import NiftiIO
    from fast_nnunet_amd.jhu import JHUPredictor
    for value, kept in ((False, False), (True, True), ('dynamic', 'dynamic'), (0, False), (1, True), (np.bool_(True), True)):
        assert compress_mode(value) is kept or compress_mode(value) == kept == 'dynamic'
        assert nnUNetPredictor(device='cuda', allow_tqdm=False, compress_on_device=value).compress_on_device == kept
    assert nnUNetPredictor(device='cuda', allow_tqdm=False).compress_on_device is False
    for bad in ('fixed', 'Dynamic', '', 2, -1, None, 1.0, [True]):
        with pytest.raises(ValueError, match='compress_on_device'):
            nnUNetPredictor(device='cuda', allow_tqdm=False, compress_on_device=bad)
        with pytest.raises(ValueError, match='compress_on_device'):
            pp.apply_postprocessing_to_folder(str(tmp_path / 'missing'), str(tmp_path / 'out'), [], [], compress_on_device=bad)
        with pytest.raises(ValueError, match='compress_on_device'):
            pp.load_postprocess_save(str(tmp_path / 'missing.nii.gz'), str(tmp_path / 'out.nii.gz'), NiftiIO(), [], [], compress_on_device=bad)
    assert os.listdir(tmp_path) == []
    with pytest.raises(NotImplementedError, match='mask encoder'):
        JHUPredictor(device='cuda', allow_tqdm=False, compress_on_device='dynamic')
    assert JHUPredictor(device='cuda', allow_tqdm=False, compress_on_device=True).compress_on_device is True
    rw = NiftiIO()
    assert device_compressor(rw, False, '.nii.gz') is None and device_compressor(rw, 'dynamic', '.nii') is None
    assert device_compressor(rw, True, '.nii.gz') == rw.compress_labels
    dynamic = device_compressor(rw, 'dynamic', '.NII.GZ')
    assert dynamic.func == rw.compress_labels and dynamic.keywords == {'tables': 'dynamic'}
    with pytest.raises(NotImplementedError, match='mask encoder'):
        device_compressor(rw, 'dynamic', '.nii.gz', 'compress_label_masks')
    with pytest.raises(ValueError, match='tables'):
        rw.compress_labels(np.zeros((2, 2, 2), np.uint8), {}, tables='best')


def test_size_condition_on_the_golden_mask(golden_dir):
    """At most 1.0 x zlib level 1, the host writer's own default; the estimate that motivated the feature gave 0.82 / 0.73."""
    voxels = gzip.decompress(open(os.path.join(golden_dir, MASK), 'rb').read())[352:]
    for elem, raw in ((1, voxels), (2, np.frombuffer(voxels, np.uint8).astype('<u2').tobytes())):
        frag, dynamic_chunks = dyn.fragment(raw, elem)
        ratio = len(frag) / len(zlib.compress(raw, 1))
        print(f'golden mask as {elem}-byte labels: {len(frag)} B in {dynamic_chunks} dynamic chunks, {ratio:.2f} x zlib level 1')
        assert deflate_ref.inflate(frag) == raw and ratio <= 1.0
