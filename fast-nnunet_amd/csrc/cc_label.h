// cc_label.h - label-aware 3-D connected components (26- or 6-connectivity, a compile-time choice; 26 is the default) by
// union-find over int32 voxel indices, gfx950: the labelling that postprocess.hip (fnn_keep_largest_components,
// fnn_remove_small_components, fnn_fill_holes) and instance.hip (fnn_instance_overlaps) share.
//
//   1. tile_merge    init + union inside a 1024-voxel tile through LDS; every voxel's global parent is the global
//                    index of its tile-local root (-1 outside every set);
//   2. cross_merge   the 13 "backward" neighbours (smaller linear index; with 6-connectivity the 3 backward face
//                    neighbours) that lie outside the voxel's tile, linked lock-free: atomicMin(&parent[a], b) with
//                    a > b, retried on the returned value (Playne & Hawick);
//   3. flatten       parent[i] = root(i);
//   4. count         size[root] += 1, aggregated per thread run and per wave before the atomic.
//
// What a voxel belongs to comes from a loader L: L::group(i, n_table) is the set of voxel i, or -1.  Two neighbours (26 or
// 6, the template's CONN) are one component iff their groups are equal and not negative.
//
// Invariants that make every phase end by construction (no spin on another workgroup's value, no recursion):
// parent[i] <= i always, and parent[] changes only through atomicMin to a smaller index, so every find walks a
// strictly decreasing chain even when it reads stale values; a union retries with a strictly smaller larger-root.  The
// root of a component is therefore its first voxel in raster order.
// Per-XCD L2s are not coherent and a CU's L1 is never refreshed by other CUs' stores: inside phases 2 and 3 every
// read of parent[] is an agent-scope relaxed atomic load (sc1), and every write an agent-scope atomic.  A stale read
// only costs a retry: the atomicMin's returned value is the truth.
// None of this depends on which neighbours are linked: CONN = 6 only offers fewer (a, b) pairs to the same local_union /
// global_union, every backward neighbour still has the smaller index, so parent[i] <= i, atomicMin-only changes and the
// agent-scope loads of phases 2 and 3 hold as written for the smaller set, and the root stays the first voxel in raster order.
#pragma once
#include "host_call.h"
#include "label_set.h"

namespace {

constexpr int CC_TILE = 1024;          // voxels per tile: 4 per thread
constexpr int CC_RUN = 16;             // consecutive voxels per thread in the size count

struct CCGeom {
    int X, Y, Z;                       // volume [X][Y][Z], X * Y * Z <= INT_MAX
    int sx, sy, sz;                    // tile = (1 << sx) x (1 << sy) x (1 << sz) = CC_TILE voxels
    int tiles_y, tiles_z;
    int n_table;                       // labels >= n_table are in no set
};

// the 13 neighbours with a smaller linear index: dx = -1 (9), dx = 0 and dy = -1 (3), dx = dy = 0 and dz = -1 (1)
__constant__ signed char c_back[13][3] = {
    {-1, -1, -1}, {-1, -1, 0}, {-1, -1, 1}, {-1, 0, -1}, {-1, 0, 0}, {-1, 0, 1}, {-1, 1, -1}, {-1, 1, 0}, {-1, 1, 1},
    {0, -1, -1}, {0, -1, 0}, {0, -1, 1}, {0, 0, -1}};
// the backward neighbours of a connectivity: N of them, neighbour k's offset along axis a is d(k, a)
template <int CONN> struct CCBack;
template <> struct CCBack<26> {
    static constexpr int N = 13;
    static __device__ __forceinline__ int d(int k, int a) { return c_back[k][a]; }
};
template <> struct CCBack<6> {                             // k = 0: dx = -1, 1: dy = -1, 2: dz = -1
    static constexpr int N = 3;
    static __device__ __forceinline__ int d(int k, int a) { return k == a ? -1 : 0; }
};

// the loader of one label map: the set of a voxel is the table's entry of its value
template <typename T>
struct CCLabelMap {
    const T *labels;
    const int *table;
    __device__ __forceinline__ int group(int i, int n_table) const { return group_of(labels, i, table, n_table); }
};

__device__ __forceinline__ int ld_agent(const int *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ int min_agent(int *p, int v) {
    return __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ int ld_wg(const int *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

// ---- union-find inside a tile (LDS, local indices; local order = global order inside a tile)
__device__ int local_find(const int *lp, int x) {
    int p = ld_wg(lp + x);
    while (p != x) { x = p; p = ld_wg(lp + x); }
    return x;
}
__device__ void local_union(int *lp, int a, int b) {
    while (true) {
        a = local_find(lp, a);
        b = local_find(lp, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(lp + a, b);
        if (old == a) return;
        a = old;                       // a was linked meanwhile: link its new parent instead (old < a)
    }
}

// ---- union-find over the volume (global indices); path halving through atomicMin keeps parent[i] <= i
__device__ int global_find(int *parent, int x) {
    while (true) {
        const int p = ld_agent(parent + x);
        if (p == x) return x;
        const int gp = ld_agent(parent + p);
        if (gp == p) return p;
        (void)min_agent(parent + x, gp);
        x = gp;
    }
}
__device__ void global_union(int *parent, int a, int b) {
    while (true) {
        a = global_find(parent, a);
        b = global_find(parent, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = min_agent(parent + a, b);
        if (old == a) return;
        a = old;
    }
}

__device__ __forceinline__ void tile_coords(const CCGeom &g, int l, int &lx, int &ly, int &lz) {
    lz = l & ((1 << g.sz) - 1);
    ly = (l >> g.sz) & ((1 << g.sy) - 1);
    lx = l >> (g.sz + g.sy);
}
__device__ __forceinline__ void tile_origin(const CCGeom &g, int &x0, int &y0, int &z0) {
    const int t = blockIdx.x;
    const int tz = t % g.tiles_z, ty = (t / g.tiles_z) % g.tiles_y, tx = t / (g.tiles_z * g.tiles_y);
    x0 = tx << g.sx; y0 = ty << g.sy; z0 = tz << g.sz;
}

// 1. init + merge inside the tile
template <class L, int CONN = 26>
__global__ __launch_bounds__(CC_THREADS) void cc_tile_merge_kernel(L src, CCGeom g, int *parent) {
    __shared__ int lp[CC_TILE];
    __shared__ int lg[CC_TILE];
    int x0, y0, z0;
    tile_origin(g, x0, y0, z0);
    const int TY = 1 << g.sy, TZ = 1 << g.sz;
    for (int l = threadIdx.x; l < CC_TILE; l += CC_THREADS) {
        int lx, ly, lz;
        tile_coords(g, l, lx, ly, lz);
        const int x = x0 + lx, y = y0 + ly, z = z0 + lz;
        int grp = -1;
        if (x < g.X && y < g.Y && z < g.Z) grp = src.group((x * g.Y + y) * g.Z + z, g.n_table);
        lg[l] = grp;
        lp[l] = grp >= 0 ? l : -1;
    }
    __syncthreads();
    for (int l = threadIdx.x; l < CC_TILE; l += CC_THREADS) {
        const int grp = lg[l];
        if (grp < 0) continue;
        int lx, ly, lz;
        tile_coords(g, l, lx, ly, lz);
#pragma unroll
        for (int k = 0; k < CCBack<CONN>::N; ++k) {
            const int nx = lx + CCBack<CONN>::d(k, 0), ny = ly + CCBack<CONN>::d(k, 1), nz = lz + CCBack<CONN>::d(k, 2);
            if (nx < 0 || ny < 0 || nz < 0 || ny >= TY || nz >= TZ) continue;
            const int nl = (nx * TY + ny) * TZ + nz;
            if (lg[nl] == grp) local_union(lp, l, nl);
        }
    }
    __syncthreads();
    for (int l = threadIdx.x; l < CC_TILE; l += CC_THREADS) {
        int lx, ly, lz;
        tile_coords(g, l, lx, ly, lz);
        const int x = x0 + lx, y = y0 + ly, z = z0 + lz;
        if (x >= g.X || y >= g.Y || z >= g.Z) continue;
        int v = -1;
        if (lg[l] >= 0) {
            int rx, ry, rz;
            tile_coords(g, local_find(lp, l), rx, ry, rz);
            v = ((x0 + rx) * g.Y + (y0 + ry)) * g.Z + (z0 + rz);
        }
        parent[(x * g.Y + y) * g.Z + z] = v;
    }
}

// 2. link across tile borders: the backward neighbours of a voxel that lie in another tile
template <class L, int CONN = 26>
__global__ __launch_bounds__(CC_THREADS) void cc_cross_merge_kernel(L src, CCGeom g, int *parent) {
    int x0, y0, z0;
    tile_origin(g, x0, y0, z0);
    const int TX = 1 << g.sx, TY = 1 << g.sy, TZ = 1 << g.sz;
    for (int l = threadIdx.x; l < CC_TILE; l += CC_THREADS) {
        int lx, ly, lz;
        tile_coords(g, l, lx, ly, lz);
        // only voxels on a tile face have neighbours in another tile (face neighbours: only on the three lower faces)
        if (lx > 0 && ly > 0 && lz > 0 && (CONN == 6 || (ly < TY - 1 && lz < TZ - 1))) continue;
        const int x = x0 + lx, y = y0 + ly, z = z0 + lz;
        if (x >= g.X || y >= g.Y || z >= g.Z) continue;
        const int i = (x * g.Y + y) * g.Z + z;
        const int grp = src.group(i, g.n_table);
        if (grp < 0) continue;
        for (int k = 0; k < CCBack<CONN>::N; ++k) {
            const int dx = CCBack<CONN>::d(k, 0), dy = CCBack<CONN>::d(k, 1), dz = CCBack<CONN>::d(k, 2);
            const int ox = lx + dx, oy = ly + dy, oz = lz + dz;
            if (ox >= 0 && oy >= 0 && oz >= 0 && oy < TY && oz < TZ && ox < TX) continue;    // inside the tile: done by 1.
            const int nx = x + dx, ny = y + dy, nz = z + dz;
            if (nx < 0 || ny < 0 || nz < 0 || ny >= g.Y || nz >= g.Z) continue;
            const int j = (nx * g.Y + ny) * g.Z + nz;
            if (src.group(j, g.n_table) == grp) global_union(parent, i, j);
        }
    }
}

// 3. every voxel points at its root
__global__ __launch_bounds__(CC_THREADS) void cc_flatten_kernel(int *parent, int n) {
    const int i = blockIdx.x * CC_THREADS + threadIdx.x;
    if (i >= n) return;
    const int p = ld_agent(parent + i);
    if (p < 0 || p == i) return;
    int r = p, q = ld_agent(parent + r);
    while (q != r) { r = q; q = ld_agent(parent + r); }
    if (r != p) (void)min_agent(parent + i, r);
}

// 4. component sizes: each thread counts a run of CC_RUN consecutive voxels, then the lanes of a wave that end on the
// same root add together - a component of 10^7 voxels costs one atomic per wave, not one per voxel
__global__ __launch_bounds__(CC_THREADS) void cc_count_kernel(const int *parent, int n, int *size) {
    const long long start = ((long long)blockIdx.x * CC_THREADS + threadIdx.x) * CC_RUN;
    int cur = -1, cnt = 0;
    for (int k = 0; k < CC_RUN; ++k) {
        const long long i = start + k;
        if (i >= n) break;
        const int r = parent[i];
        if (r < 0) continue;
        if (r != cur) {
            if (cur >= 0) atomicAdd(size + cur, cnt);
            cur = r;
            cnt = 0;
        }
        ++cnt;
    }
    const int lane = threadIdx.x & 63;
    unsigned long long act = __ballot(cur >= 0);
    while (act) {                                        // wave-uniform: every lane runs every iteration
        const int leader = __ffsll((long long)act) - 1;
        const int r = __shfl(cur, leader);
        const bool mine = cur == r;
        const int s = wave_sum(mine ? cnt : 0);
        if (lane == leader) atomicAdd(size + r, s);
        if (mine) cur = -1;
        act = __ballot(cur >= 0);
    }
}

// ---- host
// 8 x 8 x 16 tiles (28 % of the voxels on a face); thin volumes (2-D configurations: X = 1) in-plane tiles
inline CCGeom cc_geom(const int64_t shape[3], int n_tab) {
    CCGeom g{};
    g.X = (int)shape[0]; g.Y = (int)shape[1]; g.Z = (int)shape[2];
    if (g.X >= 8) { g.sx = 3; g.sy = 3; g.sz = 4; }
    else if (g.X >= 4) { g.sx = 2; g.sy = 4; g.sz = 4; }
    else { g.sx = 0; g.sy = 5; g.sz = 5; }
    g.tiles_y = (g.Y + (1 << g.sy) - 1) >> g.sy;
    g.tiles_z = (g.Z + (1 << g.sz) - 1) >> g.sz;
    g.n_table = n_tab;
    return g;
}
inline unsigned cc_tiles(const CCGeom &g) { return (unsigned)((long long)((g.X + (1 << g.sx) - 1) >> g.sx) * g.tiles_y * g.tiles_z); }
inline unsigned cc_run_blocks(int n) {
    return (unsigned)(((long long)n + (long long)CC_THREADS * CC_RUN - 1) / ((long long)CC_THREADS * CC_RUN));
}

// phases 1-3: parent[i] = the first voxel of i's component, -1 outside every set
template <class L, int CONN = 26>
void cc_label(HipCall &call, const L &src, const CCGeom &g, int n, int *parent) {
    const dim3 block(CC_THREADS);
    call.launch(cc_tile_merge_kernel<L, CONN>, dim3(cc_tiles(g)), block, 0, src, g, parent);
    call.launch(cc_cross_merge_kernel<L, CONN>, dim3(cc_tiles(g)), block, 0, src, g, parent);
    call.launch(cc_flatten_kernel, dim3(cc_vox_blocks(n)), block, 0, parent, n);
}
// phase 4 into size [n], which must be zero
inline void cc_sizes(HipCall &call, const int *parent, int n, int *size) {
    call.launch(cc_count_kernel, dim3(cc_run_blocks(n)), dim3(CC_THREADS), 0, parent, n, size);
}

}  // namespace
