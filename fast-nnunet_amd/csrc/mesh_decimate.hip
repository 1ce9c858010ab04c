// mesh_decimate.hip - fewer triangles for the surface model fnn_mesh_emit made: data-parallel rounds of quadric-error edge
// collapse, gfx950.  include/fnn.h words the rule; tests/mesh_decimate_ref.py restates it in numpy.
//
//   fnn_mesh_decimate   layout-0 points, triangles and triangle regions -> the decimated model in layout 0 or 1
//
// The work of one call:
//   lists      per vertex the triangles that hold it (count, scan, fill), sorted ascending once for the quadrics;
//   quadrics   one float64 4x4 quadric per vertex from the input mesh, summed in ascending triangle index;
//   a round    lists of the live triangles; one thread per half-edge a -> b with a < b decides whether the edge is a
//              candidate, where the merged vertex goes and what the key is; best1 is an atomicMin over the two 64-bit words of
//              the key in two passes, best2 a gather over the lists; the selected edges are applied; the triangles are
//              compacted by a scan;
//   output     the referenced points by a scan, the triangles renumbered, the regions' counts.
// A slot is a half-edge: slot 3 t + c runs from corner c of triangle t to corner (c + 1) % 3.
// Two things are placed by an atomic cursor, and neither decides a byte of the result: the entries of a vertex's list (their
// order is used by the quadrics alone, and there the list is sorted first; counts, minima and existence tests do not see
// it), and the keys of the selected edges, which the host reads only in the last round to find the k-th smallest.  All other
// atomics are integer sums and minima.
#pragma clang fp contract(off)
#include "host_call.h"
#include <algorithm>
#include <climits>
#include <cmath>
#include <utility>
#include <vector>

namespace {

typedef unsigned long long u64;
constexpr int MD_THREADS = 256;
constexpr int MD_BLOCK = 1024;             // elements per block of a scan
constexpr int MD_WAVES = MD_BLOCK / 64;
constexpr int MD_MAX_REGIONS = 1024;
constexpr int MD_MAX_VALENCE = 32;         // an end with more incident triangles takes part in no collapse
constexpr int MD_MAX_ROUNDS = 128;
constexpr u64 MD_NONE = ~0ull;

struct MDMesh {
    const int *tri;                        // [T][3] live triangles
    const unsigned int *start;             // [N + 1]: list[start[v] .. start[v + 1]) are the triangles that hold v
    const int *list;                       // [3 T]
    const float *pos;                      // [N][3]
    const double *Q;                       // [N][10] = xx xy xz xw yy yz yw zz zw ww
    long long N, T;
};

// ---- exclusive scan of n unsigned values in place: block sums, a one-block scan of them, the blocks' own scans
__global__ __launch_bounds__(MD_BLOCK) void md_block_sum_kernel(const unsigned int *v, long long n, unsigned int *bsum) {
    __shared__ unsigned int wave_n[MD_WAVES];
    const long long i = (long long)blockIdx.x * MD_BLOCK + threadIdx.x;
    unsigned int x = i < n ? v[i] : 0u;
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
    if ((threadIdx.x & 63) == 0) wave_n[threadIdx.x >> 6] = x;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned int t = 0;
        for (int k = 0; k < MD_WAVES; ++k) t += wave_n[k];
        bsum[blockIdx.x] = t;
    }
}

__global__ __launch_bounds__(MD_BLOCK) void md_scan_kernel(unsigned int *v, long long n, const unsigned int *bsum) {
    __shared__ unsigned int wave_sum[MD_WAVES];
    __shared__ unsigned int carry;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // bsum == NULL: one block walks the whole array; else every block scans its own 1024 values after bsum[block]
    if (threadIdx.x == 0) carry = bsum ? bsum[blockIdx.x] : 0u;
    __syncthreads();
    const long long first = bsum ? (long long)blockIdx.x * MD_BLOCK : 0, last = bsum ? (first + MD_BLOCK < n ? first + MD_BLOCK : n) : n;
    for (long long base = first; base < last; base += MD_BLOCK) {
        const long long i = base + threadIdx.x;
        const unsigned int own = i < last ? v[i] : 0u;
        unsigned int x = own;
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned int u = __shfl_up(x, o);
            if (lane >= o) x += u;
        }
        if (lane == 63) wave_sum[wave] = x;
        __syncthreads();
        unsigned int before = carry;
        for (int k = 0; k < wave; ++k) before += wave_sum[k];
        if (i < last) v[i] = before + x - own;
        __syncthreads();
        if (threadIdx.x == MD_BLOCK - 1) carry = before + x;
        __syncthreads();
    }
}

// ---- the input: every index inside the points, every region inside the regions
__global__ __launch_bounds__(MD_THREADS) void md_check_kernel(const int *cells, const unsigned short *cell_region, long long T, long long N, int n_regions,
                                                               unsigned int *bad) {
    const long long t = (long long)blockIdx.x * MD_THREADS + threadIdx.x;
    if (t >= T) return;
    const int a = cells[3 * t], b = cells[3 * t + 1], c = cells[3 * t + 2];
    if (a < 0 || a >= N || b < 0 || b >= N || c < 0 || c >= N || a == b || b == c || a == c || (int)cell_region[t] >= n_regions) atomicOr(bad, 1u);
}

// ---- a round's blank state: no triangle counted, nothing merged, no key seen
__global__ __launch_bounds__(MD_THREADS) void md_init_kernel(long long N, unsigned int *cnt, unsigned int *cur, int *remap, u64 *best1a, u64 *best1b,
                                                              unsigned int *counters) {
    const long long v = (long long)blockIdx.x * MD_THREADS + threadIdx.x;
    if (v == 0) { counters[0] = 0u; counters[1] = 0u; }
    if (v > N) return;
    cnt[v] = 0u;                                                     // [N + 1]
    if (v == N) return;
    cur[v] = 0u;
    remap[v] = (int)v;
    best1a[v] = MD_NONE;
    best1b[v] = MD_NONE;
}

__global__ __launch_bounds__(MD_THREADS) void md_valence_kernel(const int *tri, long long slots, unsigned int *cnt) {
    const long long s = (long long)blockIdx.x * MD_THREADS + threadIdx.x;
    if (s < slots) atomicAdd(cnt + tri[s], 1u);
}

__global__ __launch_bounds__(MD_THREADS) void md_fill_kernel(const int *tri, long long slots, const unsigned int *start, unsigned int *cur, int *list) {
    const long long s = (long long)blockIdx.x * MD_THREADS + threadIdx.x;
    if (s >= slots) return;
    const int v = tri[s];
    list[start[v] + atomicAdd(cur + v, 1u)] = (int)(s / 3);
}

__global__ __launch_bounds__(MD_THREADS) void md_sort_kernel(long long N, const unsigned int *start, int *list) {
    const long long v = (long long)blockIdx.x * MD_THREADS + threadIdx.x;
    if (v >= N) return;
    const long long lo = start[v], hi = start[v + 1];
    for (long long i = lo + 1; i < hi; ++i) {
        const int key = list[i];
        long long j = i - 1;
        while (j >= lo && list[j] > key) { list[j + 1] = list[j]; --j; }
        list[j + 1] = key;
    }
}

// (b - a) x (c - a) of float32 points in float64, every product and difference rounded on its own
__device__ __forceinline__ void md_normal(double ax, double ay, double az, double bx, double by, double bz, double cx, double cy, double cz, double &nx,
                                          double &ny, double &nz) {
    const double ux = bx - ax, uy = by - ay, uz = bz - az, vx = cx - ax, vy = cy - ay, vz = cz - az;
    const double p0 = uy * vz, p1 = uz * vy, p2 = uz * vx, p3 = ux * vz, p4 = ux * vy, p5 = uy * vx;
    nx = p0 - p1;
    ny = p2 - p3;
    nz = p4 - p5;
}

// ---- the quadric of every vertex of the input mesh: its triangles in ascending index
__global__ __launch_bounds__(MD_THREADS) void md_quadric_kernel(MDMesh m, double *Q) {
    const long long v = (long long)blockIdx.x * MD_THREADS + threadIdx.x;
    if (v >= m.N) return;
    double q0 = 0, q1 = 0, q2 = 0, q3 = 0, q4 = 0, q5 = 0, q6 = 0, q7 = 0, q8 = 0, q9 = 0;
    for (unsigned int i = m.start[v]; i < m.start[v + 1]; ++i) {
        const int *t = m.tri + 3 * (size_t)m.list[i];
        const float *a = m.pos + 3 * (size_t)t[0], *b = m.pos + 3 * (size_t)t[1], *c = m.pos + 3 * (size_t)t[2];
        const double ax = a[0], ay = a[1], az = a[2];
        double nx, ny, nz;
        md_normal(ax, ay, az, b[0], b[1], b[2], c[0], c[1], c[2], nx, ny, nz);
        const double kx = nx * ax, ky = ny * ay, kz = nz * az;
        const double k = -((kx + ky) + kz);
        const double xx = nx * nx, xy = nx * ny, xz = nx * nz, xw = nx * k, yy = ny * ny, yz = ny * nz, yw = ny * k, zz = nz * nz, zw = nz * k, ww = k * k;
        q0 = q0 + xx; q1 = q1 + xy; q2 = q2 + xz; q3 = q3 + xw; q4 = q4 + yy;
        q5 = q5 + yz; q6 = q6 + yw; q7 = q7 + zz; q8 = q8 + zw; q9 = q9 + ww;
    }
    double *o = Q + 10 * (size_t)v;
    o[0] = q0; o[1] = q1; o[2] = q2; o[3] = q3; o[4] = q4; o[5] = q5; o[6] = q6; o[7] = q7; o[8] = q8; o[9] = q9;
}

// float32(max(h^T Q h, 0)), h = (x, y, z, 1)
__device__ __forceinline__ float md_cost(const double (&q)[10], float fx, float fy, float fz) {
    const double x = fx, y = fy, z = fz;
    const double a0 = q[0] * x, a1 = q[1] * y, a2 = q[2] * z, r0 = ((a0 + a1) + a2) + q[3];
    const double b0 = q[1] * x, b1 = q[4] * y, b2 = q[5] * z, r1 = ((b0 + b1) + b2) + q[6];
    const double c0 = q[2] * x, c1 = q[5] * y, c2 = q[7] * z, r2 = ((c0 + c1) + c2) + q[8];
    const double d0 = q[3] * x, d1 = q[6] * y, d2 = q[8] * z, r3 = ((d0 + d1) + d2) + q[9];
    const double e0 = x * r0, e1 = y * r1, e2 = z * r2;
    const double c = ((e0 + e1) + e2) + r3;
    return (float)(c > 0.0 ? c : 0.0);
}

__device__ __forceinline__ unsigned int md_hash(unsigned int u, unsigned int v, unsigned int round) {
    unsigned int x = (u * 0x9E3779B1u) ^ (v * 0x85EBCA77u) ^ (round * 0xC2B2AE3Du);
    x ^= x >> 16;
    x *= 0x85EBCA6Bu;
    x ^= x >> 13;
    x *= 0xC2B2AE35u;
    return x ^ (x >> 16);
}

__device__ __forceinline__ bool md_has(const int *tri, int t, int w) {
    const int *x = tri + 3 * (size_t)t;
    return x[0] == w || x[1] == w || x[2] == w;
}

// does a surviving triangle around `end` turn its normal when `end` moves to (px, py, pz)?
__device__ __forceinline__ bool md_turns(const MDMesh &m, int end, int other, double px, double py, double pz) {
    for (unsigned int i = m.start[end]; i < m.start[end + 1]; ++i) {
        const int *x = m.tri + 3 * (size_t)m.list[i];
        const int x0 = x[0], x1 = x[1], x2 = x[2];
        if (x0 == other || x1 == other || x2 == other) continue;
        const float *a = m.pos + 3 * (size_t)x0, *b = m.pos + 3 * (size_t)x1, *c = m.pos + 3 * (size_t)x2;
        const double ax = a[0], ay = a[1], az = a[2], bx = b[0], by = b[1], bz = b[2], cx = c[0], cy = c[1], cz = c[2];
        double nx, ny, nz, mx, my, mz;
        md_normal(ax, ay, az, bx, by, bz, cx, cy, cz, nx, ny, nz);
        md_normal(x0 == end ? px : ax, x0 == end ? py : ay, x0 == end ? pz : az, x1 == end ? px : bx, x1 == end ? py : by, x1 == end ? pz : bz,
                  x2 == end ? px : cx, x2 == end ? py : cy, x2 == end ? pz : cz, mx, my, mz);
        const double d0 = nx * mx, d1 = ny * my, d2 = nz * mz;
        const double dot = (d0 + d1) + d2;
        if (!(dot > 0.0)) return true;
    }
    return false;
}

// ---- one thread per slot: is the edge a candidate, where does the merged vertex go, what is the key
// w1 = cost bits << 32 | hash32, w2 = a << 32 | b, MD_NONE for no candidate; choice 0 midpoint, 1 p[a], 2 p[b]
__global__ __launch_bounds__(MD_THREADS) void md_candidate_kernel(MDMesh m, unsigned int round, u64 *w1, u64 *w2, unsigned char *choice, u64 *best1a,
                                                                   unsigned int *counters) {
    const long long s = (long long)blockIdx.x * MD_THREADS + threadIdx.x;
    bool ok = false;
    u64 k1 = MD_NONE, k2 = MD_NONE;
    int a = 0, b = 0;
    if (s < 3 * m.T) {
        const long long t = s / 3;
        const int c = (int)(s - 3 * t);
        a = m.tri[s];
        b = m.tri[3 * t + (c + 1) % 3];
        const int c1 = m.tri[3 * t + (c + 2) % 3];
        if (a < b) {
            const unsigned int sa = m.start[a], ea = m.start[a + 1], sb = m.start[b], eb = m.start[b + 1];
            if (ea - sa <= (unsigned)MD_MAX_VALENCE && eb - sb <= (unsigned)MD_MAX_VALENCE) {
                // exactly one triangle runs a -> b (this one) and exactly one b -> a; c2 is the corner opposite in that one
                int fwd = 0, rev = 0, c2 = -1;
                for (unsigned int i = sa; i < ea; ++i) {
                    const int *x = m.tri + 3 * (size_t)m.list[i];
                    const int x0 = x[0], x1 = x[1], x2 = x[2];
                    fwd += (x0 == a && x1 == b) || (x1 == a && x2 == b) || (x2 == a && x0 == b);
                    if (x0 == b && x1 == a) { ++rev; c2 = x2; }
                    else if (x1 == b && x2 == a) { ++rev; c2 = x0; }
                    else if (x2 == b && x0 == a) { ++rev; c2 = x1; }
                }
                ok = fwd == 1 && rev == 1 && c1 != c2;
                if (ok) ok = m.start[c1 + 1] - m.start[c1] > 3u && m.start[c2 + 1] - m.start[c2] > 3u;
                // the link condition: no third vertex is a neighbour of both ends
                for (unsigned int i = sa; ok && i < ea; ++i) {
                    const int *x = m.tri + 3 * (size_t)m.list[i];
                    for (int j = 0; ok && j < 3; ++j) {
                        const int w = x[j];
                        if (w == a || w == b || w == c1 || w == c2) continue;
                        for (unsigned int q = sb; q < eb; ++q)
                            if (md_has(m.tri, m.list[q], w)) { ok = false; break; }
                    }
                }
                if (ok) {
                    double qs[10];
#pragma unroll
                    for (int k = 0; k < 10; ++k) qs[k] = m.Q[10 * (size_t)a + k] + m.Q[10 * (size_t)b + k];
                    const float *pa = m.pos + 3 * (size_t)a, *pb = m.pos + 3 * (size_t)b;
                    const float ax = pa[0], ay = pa[1], az = pa[2], bx = pb[0], by = pb[1], bz = pb[2];
                    const float sx = ax + bx, sy = ay + by, sz = az + bz;
                    float px = sx * 0.5f, py = sy * 0.5f, pz = sz * 0.5f;
                    float cost = md_cost(qs, px, py, pz);
                    int ch = 0;
                    const float ca = md_cost(qs, ax, ay, az);
                    if (ca < cost) { cost = ca; ch = 1; px = ax; py = ay; pz = az; }
                    const float cb = md_cost(qs, bx, by, bz);
                    if (cb < cost) { cost = cb; ch = 2; px = bx; py = by; pz = bz; }
                    ok = !md_turns(m, a, b, px, py, pz) && !md_turns(m, b, a, px, py, pz);
                    if (ok) {
                        k1 = ((u64)__float_as_uint(cost) << 32) | (u64)md_hash((unsigned int)a, (unsigned int)b, round);
                        k2 = ((u64)(unsigned int)a << 32) | (u64)(unsigned int)b;
                        choice[s] = (unsigned char)ch;
                    }
                }
            }
        }
        w1[s] = k1;
        w2[s] = k2;
    }
    if (ok) {
        atomicMin(best1a + a, k1);
        atomicMin(best1a + b, k1);
    }
    const u64 vote = __ballot(ok);
    if ((threadIdx.x & 63) == 0 && vote) atomicAdd(counters, (unsigned int)__popcll(vote));
}

// ---- the second word of best1: the smallest w2 among the candidates that hold the smallest w1
__global__ __launch_bounds__(MD_THREADS) void md_best1b_kernel(long long slots, const u64 *w1, const u64 *w2, const u64 *best1a, u64 *best1b) {
    const long long s = (long long)blockIdx.x * MD_THREADS + threadIdx.x;
    if (s >= slots) return;
    const u64 k1 = w1[s];
    if (k1 == MD_NONE) return;
    const u64 k2 = w2[s];
    const int a = (int)(k2 >> 32), b = (int)(k2 & 0xFFFFFFFFull);
    if (best1a[a] == k1) atomicMin(best1b + a, k2);
    if (best1a[b] == k1) atomicMin(best1b + b, k2);
}

// ---- best2: the smallest best1 over a vertex and its neighbours
__global__ __launch_bounds__(MD_THREADS) void md_best2_kernel(MDMesh m, const u64 *best1a, const u64 *best1b, u64 *best2a, u64 *best2b) {
    const long long v = (long long)blockIdx.x * MD_THREADS + threadIdx.x;
    if (v >= m.N) return;
    const unsigned int lo = m.start[v], hi = m.start[v + 1];
    u64 m1 = best1a[v];
    for (unsigned int i = lo; i < hi; ++i) {
        const int *x = m.tri + 3 * (size_t)m.list[i];
        for (int j = 0; j < 3; ++j) { const u64 k = best1a[x[j]]; m1 = k < m1 ? k : m1; }
    }
    u64 m2 = MD_NONE;
    if (m1 != MD_NONE) {
        if (best1a[v] == m1) m2 = best1b[v];
        for (unsigned int i = lo; i < hi; ++i) {
            const int *x = m.tri + 3 * (size_t)m.list[i];
            for (int j = 0; j < 3; ++j)
                if (best1a[x[j]] == m1) { const u64 k = best1b[x[j]]; m2 = k < m2 ? k : m2; }
        }
    }
    best2a[v] = m1;
    best2b[v] = m2;
}

__device__ __forceinline__ bool md_selected(long long s, const u64 *w1, const u64 *w2, const u64 *best2a, const u64 *best2b, u64 &k1, u64 &k2) {
    k1 = w1[s];
    if (k1 == MD_NONE) return false;
    k2 = w2[s];
    const int a = (int)(k2 >> 32), b = (int)(k2 & 0xFFFFFFFFull);
    return best2a[a] == k1 && best2b[a] == k2 && best2a[b] == k1 && best2b[b] == k2;
}

// ---- the keys of the selected edges, for the host to cut the last round; counters[1]: how many
__global__ __launch_bounds__(MD_THREADS) void md_select_kernel(long long slots, const u64 *w1, const u64 *w2, const u64 *best2a, const u64 *best2b,
                                                                u64 *keys, unsigned int cap, unsigned int *counters) {
    const long long s = (long long)blockIdx.x * MD_THREADS + threadIdx.x;
    u64 k1 = MD_NONE, k2 = MD_NONE;
    const bool sel = s < slots && md_selected(s, w1, w2, best2a, best2b, k1, k2);
    // one atomicAdd per wave: its first selected lane takes room for all of them
    const u64 vote = __ballot(sel);
    if (!vote) return;
    const int lane = threadIdx.x & 63, first = __ffsll((long long)vote) - 1;
    unsigned int base = 0;
    if (lane == first) base = atomicAdd(counters + 1, (unsigned int)__popcll(vote));
    base = __shfl(base, first);
    if (!sel) return;
    const unsigned int i = base + (unsigned int)__popcll(vote & ((1ull << lane) - 1ull));
    if (i < cap) { keys[2 * (size_t)i] = k1; keys[2 * (size_t)i + 1] = k2; }
}

// ---- apply the selected edges whose key is at most (t1, t2): b merges into a
__global__ __launch_bounds__(MD_THREADS) void md_apply_kernel(long long slots, const u64 *w1, const u64 *w2, const unsigned char *choice, const u64 *best2a,
                                                               const u64 *best2b, u64 t1, u64 t2, float *pos, double *Q, int *remap) {
    const long long s = (long long)blockIdx.x * MD_THREADS + threadIdx.x;
    if (s >= slots) return;
    u64 k1, k2;
    if (!md_selected(s, w1, w2, best2a, best2b, k1, k2)) return;
    if (k1 > t1 || (k1 == t1 && k2 > t2)) return;
    const int a = (int)(k2 >> 32), b = (int)(k2 & 0xFFFFFFFFull);
    float *pa = pos + 3 * (size_t)a;
    const float *pb = pos + 3 * (size_t)b;
    const int ch = choice[s];
    if (ch == 0) {
        const float sx = pa[0] + pb[0], sy = pa[1] + pb[1], sz = pa[2] + pb[2];
        pa[0] = sx * 0.5f; pa[1] = sy * 0.5f; pa[2] = sz * 0.5f;
    } else if (ch == 2) {
        pa[0] = pb[0]; pa[1] = pb[1]; pa[2] = pb[2];
    }
#pragma unroll
    for (int k = 0; k < 10; ++k) Q[10 * (size_t)a + k] = Q[10 * (size_t)a + k] + Q[10 * (size_t)b + k];
    remap[b] = a;
}

// ---- the triangles after the merges; alive[t]: its corners are still three vertices
__global__ __launch_bounds__(MD_THREADS) void md_retri_kernel(int *tri, long long T, const int *remap, unsigned int *alive) {
    const long long t = (long long)blockIdx.x * MD_THREADS + threadIdx.x;
    if (t > T) return;
    if (t == T) { alive[T] = 0u; return; }
    const int a = remap[tri[3 * t]], b = remap[tri[3 * t + 1]], c = remap[tri[3 * t + 2]];
    tri[3 * t] = a; tri[3 * t + 1] = b; tri[3 * t + 2] = c;
    alive[t] = a != b && b != c && a != c;
}

__global__ __launch_bounds__(MD_THREADS) void md_compact_kernel(const int *tri, const unsigned short *reg, long long T, const unsigned int *before, int *tri_out,
                                                                 unsigned short *reg_out) {
    const long long t = (long long)blockIdx.x * MD_THREADS + threadIdx.x;
    if (t >= T) return;
    const int a = tri[3 * t], b = tri[3 * t + 1], c = tri[3 * t + 2];
    if (a == b || b == c || a == c) return;
    const size_t o = before[t];
    tri_out[3 * o] = a; tri_out[3 * o + 1] = b; tri_out[3 * o + 2] = c;
    reg_out[o] = reg[t];
}

// ---- output
__global__ __launch_bounds__(MD_THREADS) void md_mark_kernel(const int *tri, long long slots, unsigned int *used) {
    const long long s = (long long)blockIdx.x * MD_THREADS + threadIdx.x;
    if (s < slots) used[tri[s]] = 1u;
}

__device__ __forceinline__ unsigned int md_word(unsigned int v, int big_endian) { return big_endian ? __builtin_bswap32(v) : v; }

// before[v]: the surviving points before v; before[v + 1] - before[v]: v survives
__global__ __launch_bounds__(MD_THREADS) void md_out_points_kernel(const float *pos, long long N, const unsigned int *before, int layout, unsigned int *out) {
    const long long v = (long long)blockIdx.x * MD_THREADS + threadIdx.x;
    if (v >= N) return;
    const size_t o = before[v];
    if (before[v + 1] == o) return;
    for (int k = 0; k < 3; ++k) out[3 * o + k] = md_word(__float_as_uint(pos[3 * v + k]), layout);
}

__global__ __launch_bounds__(MD_THREADS) void md_out_cells_kernel(const int *tri, const unsigned short *reg, long long T, const unsigned int *before, int layout,
                                                                   unsigned int *cells, unsigned short *cell_region, u64 *region_count) {
    const long long t = (long long)blockIdx.x * MD_THREADS + threadIdx.x;
    if (t >= T) return;
    const unsigned int a = before[tri[3 * t]], b = before[tri[3 * t + 1]], c = before[tri[3 * t + 2]];
    const unsigned short r = reg[t];
    if (layout) {
        ((uint4 *)cells)[t] = make_uint4(md_word(3u, 1), md_word(a, 1), md_word(b, 1), md_word(c, 1));
        cell_region[t] = (unsigned short)__builtin_bswap16(r);
    } else {
        cells[3 * t] = a; cells[3 * t + 1] = b; cells[3 * t + 2] = c;
        cell_region[t] = r;
    }
    // triangles come region after region: a wave of one region adds once
    const unsigned short r0 = (unsigned short)__shfl((int)r, 0);
    const u64 lanes = __ballot(1), same = __ballot(r == r0);
    if (same != lanes) atomicAdd(region_count + r, 1ull);
    else if ((threadIdx.x & 63) == 0) atomicAdd(region_count + r0, (u64)__popcll(lanes));
}

// the surviving points before every region's first point
__global__ __launch_bounds__(MD_THREADS) void md_offsets_kernel(const long long *offsets, int n, const unsigned int *before, u64 *out) {
    const int r = blockIdx.x * MD_THREADS + threadIdx.x;
    if (r < n) out[r] = before[offsets[r]];
}

// ---- host
unsigned md_grid(long long n, int per = MD_THREADS) { return (unsigned)((n + per - 1) / per > 0 ? (n + per - 1) / per : 1); }

// exclusive scan of v[0, n) in place; bsum has room for a value per 1024 of them
void md_scan(HipCall &call, unsigned int *v, long long n, unsigned int *bsum) {
    const unsigned blocks = md_grid(n, MD_BLOCK);
    if (blocks == 1) {
        call.launch(md_scan_kernel, dim3(1), dim3(MD_BLOCK), 0, v, n, (const unsigned int *)nullptr);
        return;
    }
    call.launch(md_block_sum_kernel, dim3(blocks), dim3(MD_BLOCK), 0, (const unsigned int *)v, n, bsum);
    call.launch(md_scan_kernel, dim3(1), dim3(MD_BLOCK), 0, bsum, (long long)blocks, (const unsigned int *)nullptr);
    call.launch(md_scan_kernel, dim3(blocks), dim3(MD_BLOCK), 0, v, n, (const unsigned int *)bsum);
}

struct MDWork {
    DevBuf tri[2], reg[2], pos, Q, start, cur, remap, list, w1, w2, choice, best, keys, alive, bsum, small;
    bool alloc(size_t N, size_t T, size_t R) {
        const size_t most = (N > T ? N : T) + 1;
        return tri[0].alloc(12 * T) && tri[1].alloc(12 * T) && reg[0].alloc(2 * T) && reg[1].alloc(2 * T) && pos.alloc(12 * N) && Q.alloc(80 * N) &&
               start.alloc(4 * (N + 1)) && cur.alloc(4 * N) && remap.alloc(4 * N) && list.alloc(12 * T) && w1.alloc(24 * T) && w2.alloc(24 * T) &&
               choice.alloc(3 * T) && best.alloc(32 * N) && keys.alloc(16 * (N / 2 + 1)) && alive.alloc(4 * (T + 1)) &&
               bsum.alloc(4 * ((most + MD_BLOCK - 1) / MD_BLOCK)) && small.alloc(16 + 24 * (R + 1));
    }
};

// the lists of the live triangles in tri[0, T): start by a scan of the valences, list by a cursor
void md_lists(HipCall &call, MDWork &k, const int *tri, long long N, long long T, bool sorted) {
    unsigned int *start = k.start.as<unsigned int>();
    call.launch(md_valence_kernel, dim3(md_grid(3 * T)), dim3(MD_THREADS), 0, tri, 3 * T, start);
    md_scan(call, start, N + 1, k.bsum.as<unsigned int>());
    call.launch(md_fill_kernel, dim3(md_grid(3 * T)), dim3(MD_THREADS), 0, tri, 3 * T, (const unsigned int *)start, k.cur.as<unsigned int>(), k.list.as<int>());
    if (sorted) call.launch(md_sort_kernel, dim3(md_grid(N)), dim3(MD_THREADS), 0, N, (const unsigned int *)start, k.list.as<int>());
}

}  // namespace

extern "C" int fnn_mesh_decimate(const float *points, int64_t n, const int32_t *cells, const uint16_t *cell_region, int64_t t,
                                 const int64_t *point_offsets, int n_regions, double decimation_factor, int layout, void *out_points,
                                 int64_t cap_points, void *out_cells, int64_t cap_cells, void *out_cell_region, int64_t *counts, int64_t status[4],
                                 void *stream) {
    const char *who = "fnn_mesh_decimate";
    if (!point_offsets || !counts || !status) return fnn_failf(FNN_E_INVALID, "%s: NULL argument", who);
    if (n < 0 || t < 0) return fnn_failf(FNN_E_INVALID, "%s: a count is negative", who);
    if (n_regions < 0 || n_regions > MD_MAX_REGIONS) return fnn_failf(FNN_E_INVALID, "%s: n_regions must be 0..%d", who, MD_MAX_REGIONS);
    if (!(decimation_factor >= 0.0 && decimation_factor < 1.0)) return fnn_failf(FNN_E_INVALID, "%s: decimation_factor must lie in [0, 1)", who);
    if (layout != 0 && layout != 1) return fnn_failf(FNN_E_INVALID, "%s: unknown layout", who);
    if (cap_points < 0 || cap_cells < 0) return fnn_failf(FNN_E_INVALID, "%s: a cap is negative", who);
    bool rising = point_offsets[0] == 0 && point_offsets[n_regions] == n;
    for (int r = 0; r < n_regions; ++r) rising = rising && point_offsets[r] <= point_offsets[r + 1];
    if (!rising) return fnn_failf(FNN_E_INVALID, "%s: point_offsets must rise from 0 to n", who);
    if (t > 0 && n_regions == 0) return fnn_failf(FNN_E_INVALID, "%s: triangles without a region", who);
    if (n > INT_MAX || t > INT_MAX / 3) return fnn_failf(FNN_E_UNSUPPORTED, "%s: more than 2^31 - 1 points or triangle corners", who);
    for (int k = 0; k < n_regions * 2; ++k) counts[k] = 0;
    for (int k = 0; k < 4; ++k) status[k] = 0;
    if (t == 0) return FNN_OK;
    if (((uintptr_t)points & 3) || ((uintptr_t)cells & 3) || ((uintptr_t)cell_region & 1))
        return fnn_failf(FNN_E_INVALID, "%s: points and cells must be 4-byte and cell_region 2-byte aligned", who);
    if (((uintptr_t)out_points & 3) || ((uintptr_t)out_cells & (layout ? 15 : 3)) || ((uintptr_t)out_cell_region & 1))
        return fnn_failf(FNN_E_INVALID, "%s: out_points must be 4-byte, out_cells %d-byte and out_cell_region 2-byte aligned", who, layout ? 16 : 4);
    if (int rc = fnn_need_dev(who, {points, cells, cell_region, out_points, out_cells, out_cell_region}, "device pointers for the model and the result")) return rc;

    const long long N = n, T = t;
    const long long target = (long long)std::ceil((1.0 - decimation_factor) * (double)T);
    HipCall call(stream);
    if (decimation_factor == 0.0 && layout == 0) {                   // the input, byte for byte: copies, no kernel
        if (cap_points < N) return fnn_failf(FNN_E_INVALID, "%s: cap_points is below the number of points (%lld)", who, N);
        if (cap_cells < T) return fnn_failf(FNN_E_INVALID, "%s: cap_cells is below the number of triangles (%lld)", who, T);
        std::vector<uint16_t> hreg((size_t)T);
        call.copy(out_points, points, (size_t)N * 12, hipMemcpyDeviceToDevice);
        call.copy(out_cells, cells, (size_t)T * 12, hipMemcpyDeviceToDevice);
        call.copy(out_cell_region, cell_region, (size_t)T * 2, hipMemcpyDeviceToDevice);
        call.copy(hreg.data(), cell_region, (size_t)T * 2, hipMemcpyDeviceToHost);
        if (!call.sync()) return call.fail();
        for (int r = 0; r < n_regions; ++r) counts[2 * r] = point_offsets[r + 1] - point_offsets[r];
        for (uint16_t r : hreg) if (r < n_regions) ++counts[2 * r + 1];
        status[0] = N; status[1] = T;
        return FNN_OK;
    }

    MDWork k;
    if (!k.alloc((size_t)N, (size_t)T, (size_t)n_regions))
        return fnn_failf(FNN_E_HIP, "hipMalloc failed (%s: 144 B per point and 95 B per triangle of scratch)", who);
    // small: counters u32 [4] = candidates, selected, bad input, - | per region: triangles u64, points before it u64, its offset i64
    unsigned int *counters = k.small.as<unsigned int>();
    u64 *region_count = k.small.as<u64>(16), *region_before = k.small.as<u64>(16 + 8 * (size_t)(n_regions + 1));
    long long *dev_offsets = k.small.as<long long>(16 + 16 * (size_t)(n_regions + 1));
    call.fill(k.small.p, 0, 16 + 16 * (size_t)(n_regions + 1));
    call.copy(dev_offsets, point_offsets, 8 * (size_t)(n_regions + 1), hipMemcpyHostToDevice);
    call.launch(md_check_kernel, dim3(md_grid(T)), dim3(MD_THREADS), 0, (const int *)cells, (const unsigned short *)cell_region, T, N, n_regions, counters + 2);
    unsigned int hcnt[4] = {0, 0, 0, 0};
    call.copy(hcnt, counters, 16, hipMemcpyDeviceToHost);
    if (!call.sync()) return call.fail();
    if (hcnt[2]) return fnn_failf(FNN_E_INVALID, "%s: a triangle names a point or a region that is not there, or one point twice", who);
    call.copy(k.tri[0].p, cells, (size_t)T * 12, hipMemcpyDeviceToDevice);
    call.copy(k.reg[0].p, cell_region, (size_t)T * 2, hipMemcpyDeviceToDevice);
    call.copy(k.pos.p, points, (size_t)N * 12, hipMemcpyDeviceToDevice);

    unsigned int *start = k.start.as<unsigned int>(), *cur = k.cur.as<unsigned int>(), *alive = k.alive.as<unsigned int>();
    int *remap = k.remap.as<int>();
    u64 *best1a = k.best.as<u64>(), *best1b = best1a + N, *best2a = best1b + N, *best2b = best2a + N;
    u64 *w1 = k.w1.as<u64>(), *w2 = k.w2.as<u64>(), *keys = k.keys.as<u64>();
    unsigned char *choice = k.choice.as<unsigned char>();
    const unsigned int key_cap = (unsigned int)(N / 2 + 1);
    int live = 0;                                                    // which of tri[2] / reg[2] holds the live triangles
    long long T_now = T, rounds = 0, exhausted = 0;
    auto mesh_of = [&]() { return MDMesh{k.tri[live].as<int>(), start, k.list.as<int>(), k.pos.as<float>(), k.Q.as<double>(), N, T_now}; };
    auto init = [&]() { call.launch(md_init_kernel, dim3(md_grid(N + 1)), dim3(MD_THREADS), 0, N, start, cur, remap, best1a, best1b, counters); };

    if (T_now > target) {
        init();
        md_lists(call, k, k.tri[0].as<int>(), N, T, true);
        call.launch(md_quadric_kernel, dim3(md_grid(N)), dim3(MD_THREADS), 0, mesh_of(), k.Q.as<double>());
    }
    while (T_now > target) {
        if (rounds == MD_MAX_ROUNDS) { exhausted = 1; break; }
        const long long slots = 3 * T_now;
        const unsigned sgrid = md_grid(slots);
        int *tri = k.tri[live].as<int>();
        init();
        md_lists(call, k, tri, N, T_now, false);
        const MDMesh m = mesh_of();
        call.launch(md_candidate_kernel, dim3(sgrid), dim3(MD_THREADS), 0, m, (unsigned int)rounds, w1, w2, choice, best1a, counters);
        call.launch(md_best1b_kernel, dim3(sgrid), dim3(MD_THREADS), 0, slots, (const u64 *)w1, (const u64 *)w2, (const u64 *)best1a, best1b);
        call.launch(md_best2_kernel, dim3(md_grid(N)), dim3(MD_THREADS), 0, m, (const u64 *)best1a, (const u64 *)best1b, best2a, best2b);
        call.launch(md_select_kernel, dim3(sgrid), dim3(MD_THREADS), 0, slots, (const u64 *)w1, (const u64 *)w2, (const u64 *)best2a, (const u64 *)best2b, keys,
                    key_cap, counters);
        call.copy(hcnt, counters, 16, hipMemcpyDeviceToHost);
        if (!call.sync()) return call.fail();
        if (hcnt[0] == 0) { exhausted = 1; break; }
        long long applied = hcnt[1];
        if (applied < 1 || applied > (long long)key_cap) return fnn_failf(FNN_E_HIP, "%s: a round selected %lld edges of %u candidates", who, applied, hcnt[0]);
        u64 t1 = MD_NONE, t2 = MD_NONE;
        if (T_now - 2 * applied < target) {                           // the last round: only the smallest keys
            const long long want = (T_now - target + 1) / 2;
            std::vector<std::pair<u64, u64>> sel((size_t)applied);
            call.copy(sel.data(), keys, (size_t)applied * 16, hipMemcpyDeviceToHost);
            if (!call.sync()) return call.fail();
            std::nth_element(sel.begin(), sel.begin() + (want - 1), sel.end());
            t1 = sel[(size_t)want - 1].first;
            t2 = sel[(size_t)want - 1].second;
            applied = want;
        }
        call.launch(md_apply_kernel, dim3(sgrid), dim3(MD_THREADS), 0, slots, (const u64 *)w1, (const u64 *)w2, (const unsigned char *)choice, (const u64 *)best2a,
                    (const u64 *)best2b, t1, t2, k.pos.as<float>(), k.Q.as<double>(), remap);
        call.launch(md_retri_kernel, dim3(md_grid(T_now + 1)), dim3(MD_THREADS), 0, tri, T_now, (const int *)remap, alive);
        md_scan(call, alive, T_now + 1, k.bsum.as<unsigned int>());
        call.launch(md_compact_kernel, dim3(md_grid(T_now)), dim3(MD_THREADS), 0, (const int *)tri, (const unsigned short *)k.reg[live].as<unsigned short>(), T_now,
                    (const unsigned int *)alive, k.tri[live ^ 1].as<int>(), k.reg[live ^ 1].as<unsigned short>());
        unsigned int left = 0;
        call.copy(&left, alive + T_now, 4, hipMemcpyDeviceToHost);
        if (!call.sync()) return call.fail();
        if ((long long)left != T_now - 2 * applied) return fnn_failf(FNN_E_HIP, "%s: %lld merges left %u of %lld triangles", who, applied, left, T_now);
        live ^= 1;
        T_now = left;
        ++rounds;
    }

    // the surviving points: start[] is free now and holds the marks, then the points before every point
    const int *tri = k.tri[live].as<int>();
    call.fill(start, 0, 4 * (size_t)(N + 1));
    call.launch(md_mark_kernel, dim3(md_grid(3 * T_now)), dim3(MD_THREADS), 0, tri, 3 * T_now, start);
    md_scan(call, start, N + 1, k.bsum.as<unsigned int>());
    unsigned int n_out = 0;
    call.copy(&n_out, start + N, 4, hipMemcpyDeviceToHost);
    if (!call.sync()) return call.fail();
    if (cap_points < (long long)n_out) return fnn_failf(FNN_E_INVALID, "%s: cap_points is below the number of points (%u)", who, n_out);
    if (cap_cells < T_now) return fnn_failf(FNN_E_INVALID, "%s: cap_cells is below the number of triangles (%lld)", who, T_now);
    call.launch(md_out_points_kernel, dim3(md_grid(N)), dim3(MD_THREADS), 0, (const float *)k.pos.as<float>(), N, (const unsigned int *)start, layout,
                (unsigned int *)out_points);
    call.launch(md_out_cells_kernel, dim3(md_grid(T_now)), dim3(MD_THREADS), 0, tri, (const unsigned short *)k.reg[live].as<unsigned short>(), T_now,
                (const unsigned int *)start, layout, (unsigned int *)out_cells, (unsigned short *)out_cell_region, region_count);
    call.launch(md_offsets_kernel, dim3(md_grid(n_regions + 1)), dim3(MD_THREADS), 0, (const long long *)dev_offsets, n_regions + 1, (const unsigned int *)start,
                region_before);
    std::vector<u64> hreg(2 * (size_t)(n_regions + 1));
    call.copy(hreg.data(), region_count, 16 * (size_t)(n_regions + 1), hipMemcpyDeviceToHost);
    if (!call.sync()) return call.fail();
    for (int r = 0; r < n_regions; ++r) {
        counts[2 * r] = (int64_t)(hreg[(size_t)(n_regions + 1) + r + 1] - hreg[(size_t)(n_regions + 1) + r]);
        counts[2 * r + 1] = (int64_t)hreg[r];
    }
    status[0] = n_out; status[1] = T_now; status[2] = rounds; status[3] = exhausted;
    return FNN_OK;
}
