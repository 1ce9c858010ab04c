"""tests/mesh_decimate_ref.py, the numpy statement of fnn_mesh_decimate's rule, pinned by properties that do not come from
it: the result of every scenario of the GPU test is a consistently oriented triangle soup without degenerate or repeated
triangles, it meets its target unless it says it could not, a cuboid keeps its volume and its faces exactly, and an
ellipsoid's volume stays inside a sanity cap (1 % at d = 0.2, 10 % at d = 0.9; the rule moves it by 0 % and 3.4 %)."""
import math

import numpy as np
import pytest

import mesh_decimate_cases as mc
import mesh_decimate_ref as dr


def _case(name):
    return [k for k, i in enumerate(mc.IDS) if i.startswith(name)]


@pytest.mark.parametrize('k', range(len(mc.CASES)), ids=mc.IDS)
def test_the_result_is_oriented_simple_and_at_its_target(k):
    src, out = mc.surface(k), mc.decimated(k)
    t, n = out['triangles'].astype(np.int64), len(out['points'])
    d = np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])
    assert np.array_equal(np.sort(d[:, 0] * n + d[:, 1]), np.sort(d[:, 1] * n + d[:, 0]))      # (a, b) as often as (b, a)
    assert not ((t[:, 0] == t[:, 1]) | (t[:, 1] == t[:, 2]) | (t[:, 0] == t[:, 2])).any()
    first = np.argmin(t, 1)[:, None]
    rolled = np.take_along_axis(t, (first + np.arange(3)) % 3, 1)                              # every triangle from its smallest corner
    assert len(np.unique(rolled, axis=0)) == len(t)
    target = math.ceil((1.0 - mc.CASES[k][4]) * len(src['triangles']))
    assert out['target'] == target
    assert out['exhausted'] in (0, 1) and 0 <= out['rounds'] <= dr.MAX_ROUNDS
    if out['exhausted']:
        assert len(t) > target
    else:
        assert len(t) in (target, target - 1)
    # every point is referenced, regions stay contiguous and in order, counts add up
    assert np.array_equal(np.unique(t), np.arange(n))
    assert np.all(np.diff(out['triangle_region'].astype(np.int64)) >= 0)
    assert out['counts'][:, 0].sum() == n and out['counts'][:, 1].sum() == len(t)
    off = np.concatenate([[0], np.cumsum(out['counts'][:, 0])])
    for r in range(len(off) - 1):
        mine = t[out['triangle_region'] == r]
        assert mine.size == 0 or (mine.min() >= off[r] and mine.max() < off[r + 1])


def test_factor_zero_is_the_input():
    k = _case('5x7x9-touching-flipped')[0]
    src = mc.surface(k)
    out = dr.decimate_mesh(src, 0.0)
    assert out['rounds'] == 0 and out['exhausted'] == 0
    assert out['points'].tobytes() == src['points'].tobytes() and out['triangles'].tobytes() == src['triangles'].tobytes()
    assert np.array_equal(out['counts'], np.stack([src['counts'][:, 0], 2 * src['counts'][:, 1]], 1))


def test_the_irregular_maps_exhaust_and_the_regular_ones_do_not():
    assert all(mc.decimated(k)['exhausted'] == 1 for k in _case('5x7x9-checker') + _case('5x7x9-random-identity-0-0.9'))
    assert all(mc.decimated(k)['exhausted'] == 0 for k in _case('17x33x70') + _case('14x16x18') + _case('9x9x9'))


@pytest.mark.parametrize('k', _case('9x9x9-cuboid'), ids=lambda k: mc.IDS[k])
def test_a_cuboid_keeps_its_volume_and_its_faces_exactly(k):
    src, out = mc.surface(k), mc.decimated(k)
    assert len(src['triangles']) == 300 and dr.signed_volume(src['points'], src['triangles']) == 125.0
    assert dr.signed_volume(out['points'], out['triangles']) == 125.0
    p = out['points']
    assert np.all(((p == 1.5) | (p == 6.5)).any(1)) and p.min() == 1.5 and p.max() == 6.5


@pytest.mark.parametrize('d, cap', [(0.2, 0.01), (0.9, 0.10)])
def test_the_volume_of_an_ellipsoid_stays_inside_the_cap(d, cap):
    k = _case(f'14x16x18-ellipsoid-identity-0-{d}')[0]
    src, out = mc.surface(k), mc.decimated(k)
    assert len(src['triangles']) == 1648
    v0, v1 = dr.signed_volume(src['points'], src['triangles']), dr.signed_volume(out['points'], out['triangles'])
    print(f'd = {d}: volume {v0} -> {v1} ({100 * (v1 - v0) / v0:+.4f} %), {out["rounds"]} rounds')
    assert v0 > 0 and abs(v1 - v0) <= cap * v0


def test_the_hash_mixes_and_is_the_stated_one():
    a, b = np.arange(5, dtype=np.int64), np.arange(5, dtype=np.int64) + 1
    h = dr.hash32(a, b, 3)

    def scalar(u, v, r):
        x = ((u * 0x9E3779B1) ^ (v * 0x85EBCA77) ^ (r * 0xC2B2AE3D)) & 0xFFFFFFFF
        x ^= x >> 16
        x = (x * 0x85EBCA6B) & 0xFFFFFFFF
        x ^= x >> 13
        x = (x * 0xC2B2AE35) & 0xFFFFFFFF
        return x ^ (x >> 16)

    assert h.dtype == np.uint32 and h.tolist() == [scalar(int(u), int(v), 3) for u, v in zip(a, b)]
    assert len(set(h.tolist())) == 5 and not np.array_equal(h, dr.hash32(a, b, 4))
