"""The decimation of a surface model as fnn_mesh_decimate (csrc/mesh_decimate.hip) must give it, restated in numpy: rounds
of quadric-error edge collapse exactly as include/fnn.h words them - the quadrics, the candidates, the key, the staged
minima, the last round and the output.  tests/test_mesh_decimate_ref_cpu.py pins this file by properties that do not come
from it; the GPU tests compare the library with it bit for bit.  The input is what tests/mesh_ref.py's mesh() returns."""
import math

import numpy as np

MAX_VALENCE = 32          # an end with more incident triangles takes part in no collapse
MAX_ROUNDS = 128
_NONE = np.iinfo(np.int64).max


def hash32(u, v, rnd):
    """The tie-break: x = u * 0x9E3779B1 ^ v * 0x85EBCA77 ^ round * 0xC2B2AE3D, then murmur3's finaliser; all in uint32."""
    x = (u.astype(np.uint32) * np.uint32(0x9E3779B1)) ^ (v.astype(np.uint32) * np.uint32(0x85EBCA77))
    x = x ^ np.uint32((int(rnd) * 0xC2B2AE3D) & 0xFFFFFFFF)
    x = x ^ (x >> np.uint32(16))
    x = x * np.uint32(0x85EBCA6B)
    x = x ^ (x >> np.uint32(13))
    x = x * np.uint32(0xC2B2AE35)
    return x ^ (x >> np.uint32(16))


def _cross(e1, e2):
    """(e1 x e2), every product and difference rounded on its own; [..., 3] float64."""
    return np.stack([e1[..., 1] * e2[..., 2] - e1[..., 2] * e2[..., 1],
                     e1[..., 2] * e2[..., 0] - e1[..., 0] * e2[..., 2],
                     e1[..., 0] * e2[..., 1] - e1[..., 1] * e2[..., 0]], -1)


def _expand(starts, lens):
    """For item i the indices starts[i] .. starts[i] + lens[i] - 1 -> (owner of every index, the indices)."""
    lens = lens.astype(np.int64)
    owner = np.repeat(np.arange(len(lens)), lens)
    first = np.cumsum(lens) - lens
    return owner, starts[owner] + (np.arange(int(lens.sum())) - first[owner])


def quadrics(points, tri):
    """float64 [n][10] = xx xy xz xw yy yz yw zz zw ww: per vertex the sum over its triangles in ascending index of K K^T,
    K = (n, k), n = (b - a) x (c - a), k = -((nx ax + ny ay) + nz az)."""
    p = points.astype(np.float64)
    a, b, c = p[tri[:, 0]], p[tri[:, 1]], p[tri[:, 2]]
    n = _cross(b - a, c - a)
    k = -((n[:, 0] * a[:, 0] + n[:, 1] * a[:, 1]) + n[:, 2] * a[:, 2])
    K = np.concatenate([n, k[:, None]], 1)
    pairs = [(0, 0), (0, 1), (0, 2), (0, 3), (1, 1), (1, 2), (1, 3), (2, 2), (2, 3), (3, 3)]
    per_tri = np.stack([K[:, i] * K[:, j] for i, j in pairs], 1)
    vert = tri.ravel()
    order = np.argsort(vert, kind='stable')                          # by vertex, then slot = ascending triangle index
    vs, ts = vert[order], order // 3
    start = np.concatenate([[0], np.cumsum(np.bincount(vert, minlength=len(p)))])
    rank = np.arange(len(vs)) - start[vs]
    Q = np.zeros((len(p), 10))
    for r in range(int(rank.max()) + 1 if len(rank) else 0):
        m = rank == r
        Q[vs[m]] = Q[vs[m]] + per_tri[ts[m]]
    return Q


def _cost(Q, p):
    """float32(max(h^T Q h, 0)) for h = (p, 1), p float32 [m][3]."""
    x, y, z = (p[:, k].astype(np.float64) for k in range(3))
    q = Q.T
    r0 = ((q[0] * x + q[1] * y) + q[2] * z) + q[3]
    r1 = ((q[1] * x + q[4] * y) + q[5] * z) + q[6]
    r2 = ((q[2] * x + q[5] * y) + q[7] * z) + q[8]
    r3 = ((q[3] * x + q[6] * y) + q[8] * z) + q[9]
    c = ((x * r0 + y * r1) + z * r2) + r3
    with np.errstate(over='ignore'):
        return np.where(c > 0, c, 0.0).astype(np.float32)


def _round(pos, Q, tri, rnd):
    """The candidates of one round: (a, b, p float32 [m][3], rank) with rank the place of the candidate's key in the total
    order, and the undirected adjacency as sorted unique keys x * N + y."""
    N = len(pos)
    A, B, C = tri.ravel(), tri[:, [1, 2, 0]].ravel(), tri[:, [2, 0, 1]].ravel()
    val = np.bincount(A, minlength=N)
    dkey, rkey = A * N + B, B * N + A
    so = np.argsort(dkey, kind='stable')
    sk = dkey[so]
    nf = np.searchsorted(sk, dkey, 'right') - np.searchsorted(sk, dkey, 'left')
    lo = np.searchsorted(sk, rkey, 'left')
    nr = np.searchsorted(sk, rkey, 'right') - lo
    ukeys = np.unique(np.concatenate([dkey, rkey]))
    s = np.flatnonzero((A < B) & (nf == 1) & (nr == 1) & (val[A] <= MAX_VALENCE) & (val[B] <= MAX_VALENCE))
    a, b, c1, c2 = A[s], B[s], C[s], C[so[lo[s]]]
    keep = (c1 != c2) & (val[c1] > 3) & (val[c2] > 3)
    a, b = a[keep], b[keep]
    # the link condition: exactly two vertices are neighbours of both ends
    asrc, adst = ukeys // N, ukeys % N
    astart = np.concatenate([[0], np.cumsum(np.bincount(asrc, minlength=N))])
    owner, idx = _expand(astart[a], astart[a + 1] - astart[a])
    want = b[owner] * N + adst[idx]
    at = np.minimum(np.searchsorted(ukeys, want), len(ukeys) - 1)
    common = np.bincount(owner, weights=(ukeys[at] == want), minlength=len(a))
    keep = common == 2
    a, b = a[keep], b[keep]
    # the position: the cheapest of the midpoint, p[a], p[b], in this order on ties
    Qs = Q[a] + Q[b]
    cand = [(pos[a] + pos[b]) * np.float32(0.5), pos[a], pos[b]]
    p, cost = cand[0].copy(), _cost(Qs, cand[0])
    for q in cand[1:]:
        c = _cost(Qs, q)
        better = c < cost
        p[better], cost[better] = q[better], c[better]
    # no surviving triangle around an end may turn its normal
    order = np.argsort(A, kind='stable')
    vstart = np.concatenate([[0], np.cumsum(val)])
    pos64, p64 = pos.astype(np.float64), p.astype(np.float64)
    bad = np.zeros(len(a))
    for end, other in ((a, b), (b, a)):
        owner, idx = _expand(vstart[end], val[end])
        tv = tri[order[idx] // 3]
        P = pos64[tv]
        moved = np.where((tv == end[owner, None])[..., None], p64[owner][:, None, :], P)
        n0 = _cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0])
        n1 = _cross(moved[:, 1] - moved[:, 0], moved[:, 2] - moved[:, 0])
        dot = (n0[:, 0] * n1[:, 0] + n0[:, 1] * n1[:, 1]) + n0[:, 2] * n1[:, 2]
        survives = ~(tv == other[owner, None]).any(1)
        bad += np.bincount(owner, weights=survives & ~(dot > 0), minlength=len(a))
    keep = bad == 0
    a, b, p, cost = a[keep], b[keep], p[keep], cost[keep]
    rank = np.empty(len(a), np.int64)
    rank[np.lexsort((b, a, hash32(a, b, rnd), cost.view(np.uint32)))] = np.arange(len(a))
    return a, b, p, rank, ukeys


def decimate(points, triangles, triangle_region, point_offsets, decimation_factor, max_rounds=MAX_ROUNDS):
    """-> dict(points float32 [n'][3], triangles int32 [t'][3], triangle_region uint16 [t'], counts int64 [R][2] (points,
    triangles of every region), rounds, exhausted, target)."""
    d = float(decimation_factor)
    assert 0.0 <= d < 1.0
    R = len(point_offsets) - 1
    pos = np.array(points, np.float32)
    tri = np.array(triangles, np.int64).reshape(-1, 3)
    reg = np.array(triangle_region, np.uint16)
    N, T = len(pos), len(tri)
    target = int(math.ceil((1.0 - d) * T))
    rounds, exhausted = 0, 0
    if d > 0 and T:
        Q = quadrics(pos, tri)
        while len(tri) > target:
            if rounds == max_rounds:
                exhausted = 1
                break
            a, b, p, rank, ukeys = _round(pos, Q, tri, rounds)
            if len(a) == 0:
                exhausted = 1
                break
            best1 = np.full(N, _NONE)
            np.minimum.at(best1, a, rank)
            np.minimum.at(best1, b, rank)
            best2 = best1.copy()
            np.minimum.at(best2, ukeys // N, best1[ukeys % N])
            sel = np.flatnonzero((best2[a] == rank) & (best2[b] == rank))
            sel = sel[np.argsort(rank[sel])]
            if len(tri) - 2 * len(sel) < target:
                sel = sel[:(len(tri) - target + 1) // 2]
            a, b, p = a[sel], b[sel], p[sel]
            pos[a] = p
            Q[a] = Q[a] + Q[b]
            remap = np.arange(N)
            remap[b] = a
            tri = remap[tri]
            alive = (tri[:, 0] != tri[:, 1]) & (tri[:, 1] != tri[:, 2]) & (tri[:, 0] != tri[:, 2])
            assert int((~alive).sum()) == 2 * len(sel)
            tri, reg = tri[alive], reg[alive]
            rounds += 1
    used = np.zeros(N, bool)
    used[tri.ravel()] = True
    new = np.cumsum(used) - 1
    off = np.asarray(point_offsets, np.int64)
    counts = np.zeros((R, 2), np.int64)
    before = np.concatenate([[0], np.cumsum(used)])
    counts[:, 0] = before[off[1:]] - before[off[:-1]]
    counts[:, 1] = np.bincount(reg, minlength=R)[:R]
    return {'points': pos[used], 'triangles': new[tri].astype(np.int32).reshape(-1, 3), 'triangle_region': reg, 'counts': counts,
            'rounds': rounds, 'exhausted': exhausted, 'target': target}


def decimate_mesh(m, decimation_factor):
    """decimate() of a mesh_ref.mesh() result."""
    off = np.concatenate([[0], np.cumsum(m['counts'][:, 0])])
    return decimate(m['points'], m['triangles'], m['triangle_region'], off, decimation_factor)


def payload(m, layout):
    """The bytes of the three output buffers in layout 0 or 1."""
    if not layout:
        return m['points'].tobytes(), m['triangles'].tobytes(), m['triangle_region'].tobytes()
    cells = np.concatenate([np.full((len(m['triangles']), 1), 3, np.int32), m['triangles']], 1)
    return m['points'].astype('>f4').tobytes(), cells.astype('>i4').tobytes(), m['triangle_region'].astype('>u2').tobytes()


def signed_volume(points, triangles):
    p = points.astype(np.float64)
    a, b, c = p[triangles[:, 0]], p[triangles[:, 1]], p[triangles[:, 2]]
    return float((a * np.cross(b, c)).sum() / 6.0)
