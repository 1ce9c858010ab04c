// mesh.hip - the surface of every region of a label map as triangles, for a coloured 3-D model of a segmentation, gfx950.
//
//   fnn_mesh_count   per region: its vertices and faces and the [lo, hi) box of its voxels
//   fnn_mesh_emit    all regions one after another: points (world coordinates), triangles, the region of every triangle
//
// A region is a set of label values (bits[v]: one bit per region value v belongs to, as in surface.hip).  Its surface is the
// set of voxel faces between a voxel of the region and a 6-neighbour outside it (the outside of the volume included), its
// vertices the lattice corners whose 8 surrounding voxels are neither all inside nor all outside.  Faces are ordered by the
// raster index of their voxel and then by direction (-z +z -y +y -x +x), vertices by the raster index of their corner.
//
// One pass over the whole map counts the faces and finds the box of every region at once.  Everything after it walks the
// boxes of the regions that have faces, all regions in one launch: a block owns MS_BLOCK raster-consecutive corners (or
// voxels) of one region's box and finds its region by a binary search over the regions' first blocks.
//   corners   one bit per box corner (the ballots of the block's 16 waves), the vertices before every 64-bit word inside
//             its block, and the block's count; a scan of the block counts over all regions then gives
//             vertex index = block prefix + word prefix + popcount(word below the bit)
//             anywhere, with no index volume;
//   points    index-space positions (float32) and, for smoothing, the up to 6 lattice neighbours of every vertex - the
//             edge to a neighbour exists iff its 4 surrounding voxels are mixed, which the 8 voxels around the corner say;
//   smooth    Jacobi passes over the vertices, p' = p + f (m - p), every operation rounded on its own;
//   world     ((A[r][0] x + A[r][1] y) + A[r][2] z) + A[r][3] in float64, rounded once to float32;
//   faces     per block of box voxels the face count, a scan, and the two triangles of every face at
//             block prefix + rank in the block (a scan of the threads' face counts).
// No atomic cursor decides where anything is written: the same input gives the same bytes.  The only atomics are integer
// sums, minima and maxima of the counts and boxes.
#pragma clang fp contract(off)
#include "host_call.h"
#include <climits>
#include <cmath>
#include <vector>

namespace {

constexpr int MS_THREADS = 256;
constexpr int MS_MAX_REGIONS = 1024;       // 8 LDS words per region in the count kernel: 32 KiB
constexpr int MS_BLOCK = 1024;             // raster-consecutive box corners or voxels per block
constexpr int MS_WORDS = MS_BLOCK / 64;

struct MSGeom {
    int Z, Y, X;
    const unsigned long long *bits;        // [n_tab][W]: bit r of bits[v] - value v belongs to region r
    int n_tab, W;
};
// a region with faces: its voxel box, its index, its first block of box corners and of box voxels
struct MSRegion {
    int z0, y0, x0, bz, by, bx, r;
    unsigned int cblk0, vblk0;
};
struct MSIndex {
    const unsigned long long *words;       // [corner blocks][16]: bit c & 63 of word c >> 6 - box corner c is a vertex
    const unsigned int *wpre;              // [corner blocks][16]: the vertices of the block before the word
    const unsigned int *bpre;              // [corner blocks]: the vertices of all regions before the block
};
struct MSAffine { double a[3][4]; };

__device__ __forceinline__ unsigned long long ms_bits(const MSGeom &g, int v, int w) {
    return v < g.n_tab ? g.bits[(size_t)v * g.W + w] : 0ull;
}

// is voxel (z, y, x) of the region's box in the region?  Nothing outside the box is, and nothing outside it is read
template <typename T>
__device__ __forceinline__ bool ms_in(const T *seg, const MSGeom &g, const MSRegion &b, int z, int y, int x) {
    if ((unsigned)z >= (unsigned)b.bz || (unsigned)y >= (unsigned)b.by || (unsigned)x >= (unsigned)b.bx) return false;
    const int v = seg[((size_t)(b.z0 + z) * g.Y + (b.y0 + y)) * g.X + (b.x0 + x)];
    return (ms_bits(g, v, b.r >> 6) >> (b.r & 63)) & 1ull;
}

// the 8 voxels around box corner (cz, cy, cx): bit dz*4 + dy*2 + dx - voxel (cz-1+dz, cy-1+dy, cx-1+dx) is in the region
template <typename T>
__device__ __forceinline__ unsigned int ms_octants(const T *seg, const MSGeom &g, const MSRegion &b, int cz, int cy, int cx) {
    unsigned int o = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) o |= (unsigned int)ms_in<T>(seg, g, b, cz - 1 + (k >> 2), cy - 1 + ((k >> 1) & 1), cx - 1 + (k & 1)) << k;
    return o;
}

// the region whose blocks hold block blk: the last one that starts at or before it
__device__ __forceinline__ int ms_find(const MSRegion *regs, int n, unsigned int blk, bool corners) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if ((corners ? regs[mid].cblk0 : regs[mid].vblk0) <= blk) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// box corner c of region b (raster index in its corner grid) -> its vertex index among all regions
__device__ __forceinline__ int ms_vertex(const MSIndex &ix, const MSRegion &b, long long c) {
    const size_t w = (size_t)b.cblk0 * MS_WORDS + (size_t)(c >> 6);
    return (int)(ix.bpre[b.cblk0 + (unsigned int)(c >> 10)] + ix.wpre[w] + (unsigned int)__popcll(ix.words[w] & ((1ull << (c & 63)) - 1ull)));
}

// ---- faces and boxes of every region, one pass over the map
// LDS: [n_regions][8] = faces, -, lowest z, y, x, highest z, y, x.  Only voxels with a face touch it (LDS integer atomics);
// a block adds to the global words once per region it met.
template <typename T>
__global__ __launch_bounds__(MS_THREADS) void ms_count_kernel(const T *seg, MSGeom g, int n_regions, unsigned long long *gcnt, int *gbox) {
    extern __shared__ int acc[];
    for (int k = threadIdx.x; k < n_regions * 8; k += MS_THREADS) acc[k] = (k & 7) < 2 ? 0 : ((k & 7) < 5 ? INT_MAX : -1);
    __syncthreads();
    const long long n = (long long)g.Z * g.Y * g.X, stride = (long long)gridDim.x * MS_THREADS;
    const int plane = g.Y * g.X;
    for (long long i = (long long)blockIdx.x * MS_THREADS + threadIdx.x; i < n; i += stride) {
        const int z = (int)(i / plane), rem = (int)(i - (long long)z * plane), y = rem / g.X, x = rem - y * g.X;
        const int v = seg[i];
        if (v >= g.n_tab) continue;
        // the six neighbours' values; -1: outside the volume, in no region
        const int a = z > 0 ? (int)seg[i - plane] : -1, b = z < g.Z - 1 ? (int)seg[i + plane] : -1;
        const int c = y > 0 ? (int)seg[i - g.X] : -1, d = y < g.Y - 1 ? (int)seg[i + g.X] : -1;
        const int e = x > 0 ? (int)seg[i - 1] : -1, f = x < g.X - 1 ? (int)seg[i + 1] : -1;
        if (a == v && b == v && c == v && d == v && e == v && f == v) continue;
        for (int w = 0; w < g.W; ++w) {
            const unsigned long long in = g.bits[(size_t)v * g.W + w];
            if (!in) continue;
            const unsigned long long na = a < 0 ? 0ull : ms_bits(g, a, w), nb = b < 0 ? 0ull : ms_bits(g, b, w);
            const unsigned long long nc = c < 0 ? 0ull : ms_bits(g, c, w), nd = d < 0 ? 0ull : ms_bits(g, d, w);
            const unsigned long long ne = e < 0 ? 0ull : ms_bits(g, e, w), nf = f < 0 ? 0ull : ms_bits(g, f, w);
            unsigned long long s = in & ~(na & nb & nc & nd & ne & nf);
            while (s) {
                const int bit = __ffsll((long long)s) - 1;
                s &= s - 1;
                const int faces = 6 - (int)(((na >> bit) & 1) + ((nb >> bit) & 1) + ((nc >> bit) & 1) + ((nd >> bit) & 1) +
                                            ((ne >> bit) & 1) + ((nf >> bit) & 1));
                int *q = acc + (w * 64 + bit) * 8;
                atomicAdd(q, faces);
                atomicMin(q + 2, z); atomicMin(q + 3, y); atomicMin(q + 4, x);
                atomicMax(q + 5, z); atomicMax(q + 6, y); atomicMax(q + 7, x);
            }
        }
    }
    __syncthreads();
    for (int r = threadIdx.x; r < n_regions; r += MS_THREADS) {
        const int *q = acc + r * 8;
        if (q[0] == 0) continue;
        atomicAdd(gcnt + r, (unsigned long long)(unsigned int)q[0]);
        for (int k = 0; k < 3; ++k) { atomicMin(gbox + 6 * r + k, q[2 + k]); atomicMax(gbox + 6 * r + 3 + k, q[5 + k]); }
    }
}

// ---- which box corners are vertices: the bit words, the word prefixes inside the block, the block's and the region's count
template <typename T>
__global__ __launch_bounds__(MS_BLOCK) void ms_corner_kernel(const T *seg, MSGeom g, const MSRegion *regs, int n_act, unsigned long long *words,
                                                              unsigned int *wpre, unsigned int *bcnt, unsigned long long *vcnt) {
    __shared__ unsigned int wave_n[MS_WORDS];
    const int a = ms_find(regs, n_act, blockIdx.x, true);
    const MSRegion b = regs[a];
    const long long cyx = (long long)(b.by + 1) * (b.bx + 1), n_c = (long long)(b.bz + 1) * cyx;
    const long long c = (long long)(blockIdx.x - b.cblk0) * MS_BLOCK + threadIdx.x;
    bool vertex = false;
    if (c < n_c) {
        const int cz = (int)(c / cyx), rem = (int)(c - cz * cyx), cy = rem / (b.bx + 1), cx = rem - cy * (b.bx + 1);
        const unsigned int o = ms_octants<T>(seg, g, b, cz, cy, cx);
        vertex = o != 0u && o != 255u;
    }
    const unsigned long long vote = __ballot(vertex);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
        wave_n[wave] = (unsigned int)__popcll(vote);
        words[(size_t)blockIdx.x * MS_WORDS + wave] = vote;
    }
    __syncthreads();
    if (threadIdx.x < MS_WORDS) {
        unsigned int before = 0;
        for (int k = 0; k < (int)threadIdx.x; ++k) before += wave_n[k];
        wpre[(size_t)blockIdx.x * MS_WORDS + threadIdx.x] = before;
        if (threadIdx.x == MS_WORDS - 1) {
            const unsigned int total = before + wave_n[MS_WORDS - 1];
            bcnt[blockIdx.x] = total;
            if (total) atomicAdd(vcnt + a, (unsigned long long)total);
        }
    }
}

// ---- exclusive scan of per-block counts in place, one block
__global__ __launch_bounds__(MS_BLOCK) void ms_scan_kernel(unsigned int *counts, int n) {
    __shared__ unsigned int wave_sum[MS_WORDS];
    __shared__ unsigned int carry;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (int base = 0; base < n; base += MS_BLOCK) {
        const int i = base + threadIdx.x;
        const unsigned int own = i < n ? counts[i] : 0u;
        unsigned int v = own;
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned int u = __shfl_up(v, o);
            if (lane >= o) v += u;
        }
        if (lane == 63) wave_sum[wave] = v;
        __syncthreads();
        unsigned int before = carry;
        for (int k = 0; k < wave; ++k) before += wave_sum[k];
        if (i < n) counts[i] = before + v - own;
        __syncthreads();
        if (threadIdx.x == MS_BLOCK - 1) carry = before + v;
        __syncthreads();
    }
}

// ---- index-space positions of the vertices, and their lattice neighbours in the order -x +x -y +y -z +z (-1: none) when
// nbr is given: nbr[k][vertex], n vertices in all
template <typename T>
__global__ __launch_bounds__(MS_BLOCK) void ms_points_kernel(const T *seg, MSGeom g, const MSRegion *regs, int n_act, MSIndex ix, float *pos,
                                                              int *nbr, long long n) {
    const MSRegion b = regs[ms_find(regs, n_act, blockIdx.x, true)];
    const long long cyx = (long long)(b.by + 1) * (b.bx + 1), n_c = (long long)(b.bz + 1) * cyx;
    const long long c = (long long)(blockIdx.x - b.cblk0) * MS_BLOCK + threadIdx.x;
    if (c >= n_c) return;
    if (!((ix.words[(size_t)b.cblk0 * MS_WORDS + (size_t)(c >> 6)] >> (c & 63)) & 1ull)) return;
    const int cz = (int)(c / cyx), rem = (int)(c - cz * cyx), cy = rem / (b.bx + 1), cx = rem - cy * (b.bx + 1);
    const long long v = ms_vertex(ix, b, c);
    if (v >= n) return;
    pos[3 * v] = (float)(b.x0 + cx) - 0.5f;
    pos[3 * v + 1] = (float)(b.y0 + cy) - 0.5f;
    pos[3 * v + 2] = (float)(b.z0 + cz) - 0.5f;
    if (!nbr) return;
    const unsigned int o = ms_octants<T>(seg, g, b, cz, cy, cx);
    // the 4 voxels around the edge towards -x are the octants with dx = 0, and so on
    const unsigned int part[6] = {0x55u, 0xAAu, 0x33u, 0xCCu, 0x0Fu, 0xF0u};
    const long long step[6] = {-1, 1, -(long long)(b.bx + 1), (long long)(b.bx + 1), -cyx, cyx};
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const unsigned int m = o & part[k];
        nbr[(size_t)k * n + v] = (m != 0u && m != part[k]) ? ms_vertex(ix, b, c + step[k]) : -1;
    }
}

// ---- one Jacobi pass: out = p + f (m - p), m = (sum of the present neighbours in their order) * float32(1 / count)
__global__ __launch_bounds__(MS_THREADS) void ms_smooth_kernel(const float *in, const int *nbr, long long n, float f, float *out) {
    const long long v = (long long)blockIdx.x * MS_THREADS + threadIdx.x;
    if (v >= n) return;
    float sx = 0.f, sy = 0.f, sz = 0.f;
    int cnt = 0;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const int j = nbr[(size_t)k * n + v];
        if (j < 0) continue;
        sx = sx + in[3 * (size_t)j];
        sy = sy + in[3 * (size_t)j + 1];
        sz = sz + in[3 * (size_t)j + 2];
        ++cnt;
    }
    const float rcp = cnt == 1 ? 1.0f : cnt == 2 ? 0.5f : cnt == 3 ? (float)(1.0 / 3.0) : cnt == 4 ? 0.25f : cnt == 5 ? (float)(1.0 / 5.0)
                      : cnt == 6 ? (float)(1.0 / 6.0) : 0.0f;
    const float px = in[3 * v], py = in[3 * v + 1], pz = in[3 * v + 2];
    const float mx = sx * rcp, my = sy * rcp, mz = sz * rcp;
    const float dx = mx - px, dy = my - py, dz = mz - pz;
    const float tx = f * dx, ty = f * dy, tz = f * dz;
    out[3 * v] = px + tx;
    out[3 * v + 1] = py + ty;
    out[3 * v + 2] = pz + tz;
}

__device__ __forceinline__ unsigned int ms_word(unsigned int v, int big_endian) { return big_endian ? __builtin_bswap32(v) : v; }

// ---- index space -> world, float64, one rounding to float32; big_endian: the bytes of a legacy-VTK POINTS section
__global__ __launch_bounds__(MS_THREADS) void ms_world_kernel(const float *pos, long long n, MSAffine A, int big_endian, unsigned int *points) {
    const long long v = (long long)blockIdx.x * MS_THREADS + threadIdx.x;
    if (v >= n) return;
    const double x = (double)pos[3 * v], y = (double)pos[3 * v + 1], z = (double)pos[3 * v + 2];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const double xa = A.a[r][0] * x, ya = A.a[r][1] * y, za = A.a[r][2] * z;
        const double w = ((xa + ya) + za) + A.a[r][3];
        points[3 * v + r] = ms_word(__float_as_uint((float)w), big_endian);
    }
}

// the faces of box voxel i as a mask over -z +z -y +y -x +x
template <typename T>
__device__ __forceinline__ unsigned int ms_faces(const T *seg, const MSGeom &g, const MSRegion &b, long long i, long long n_box, int &z, int &y, int &x) {
    z = y = x = 0;
    if (i >= n_box) return 0u;
    const long long plane = (long long)b.by * b.bx;
    z = (int)(i / plane);
    const int rem = (int)(i - z * plane);
    y = rem / b.bx;
    x = rem - y * b.bx;
    if (!ms_in<T>(seg, g, b, z, y, x)) return 0u;
    return (unsigned int)!ms_in<T>(seg, g, b, z - 1, y, x) | (unsigned int)!ms_in<T>(seg, g, b, z + 1, y, x) << 1 |
           (unsigned int)!ms_in<T>(seg, g, b, z, y - 1, x) << 2 | (unsigned int)!ms_in<T>(seg, g, b, z, y + 1, x) << 3 |
           (unsigned int)!ms_in<T>(seg, g, b, z, y, x - 1) << 4 | (unsigned int)!ms_in<T>(seg, g, b, z, y, x + 1) << 5;
}

// ---- faces per block of MS_BLOCK raster-consecutive box voxels
template <typename T>
__global__ __launch_bounds__(MS_BLOCK) void ms_face_count_kernel(const T *seg, MSGeom g, const MSRegion *regs, int n_act, unsigned int *fcnt) {
    __shared__ unsigned int wave_n[MS_WORDS];
    const MSRegion b = regs[ms_find(regs, n_act, blockIdx.x, false)];
    const long long n_box = (long long)b.bz * b.by * b.bx, i = (long long)(blockIdx.x - b.vblk0) * MS_BLOCK + threadIdx.x;
    int z, y, x;
    unsigned int v = (unsigned int)__popc(ms_faces<T>(seg, g, b, i, n_box, z, y, x));
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    if ((threadIdx.x & 63) == 0) wave_n[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned int t = 0;
        for (int k = 0; k < MS_WORDS; ++k) t += wave_n[k];
        fcnt[blockIdx.x] = t;
    }
}

// ---- the two triangles of every face at 2 * (block prefix + rank of the face in the block)
// layout 0: cells int32 [t][3], region uint16;  layout 1: cells [t][4] = 3, a, b, c and region, all big-endian
template <typename T>
__global__ __launch_bounds__(MS_BLOCK) void ms_cells_kernel(const T *seg, MSGeom g, const MSRegion *regs, int n_act, MSIndex ix, const unsigned int *fpre,
                                                             int flip, int layout, unsigned int *cells, unsigned short *cell_region, long long n_tri) {
    __shared__ unsigned int wave_n[MS_WORDS];
    const MSRegion b = regs[ms_find(regs, n_act, blockIdx.x, false)];
    const long long n_box = (long long)b.bz * b.by * b.bx, i = (long long)(blockIdx.x - b.vblk0) * MS_BLOCK + threadIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int z, y, x;
    const unsigned int mask = ms_faces<T>(seg, g, b, i, n_box, z, y, x);
    const unsigned int own = (unsigned int)__popc(mask);
    unsigned int v = own;
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned int u = __shfl_up(v, o);
        if (lane >= o) v += u;
    }
    if (lane == 63) wave_n[wave] = v;
    __syncthreads();
    if (!mask) return;
    long long face = (long long)fpre[blockIdx.x] + v - own;
    for (int k = 0; k < wave; ++k) face += wave_n[k];
    const long long cx1 = b.bx + 1, cyx = (long long)(b.by + 1) * cx1;
    const long long c0 = (long long)z * cyx + (long long)y * cx1 + x;   // the voxel's lowest corner
    const unsigned short reg = layout ? (unsigned short)__builtin_bswap16((unsigned short)b.r) : (unsigned short)b.r;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        if (!((mask >> k) & 1u)) continue;
        // the face's corners in raster order: the side along its axis, then the two other axes
        const long long side = (k & 1) ? (k < 2 ? cyx : k < 4 ? cx1 : 1) : 0;
        const long long u1 = k < 4 ? 1 : cx1, u2 = k < 2 ? cx1 : cyx;
        const int q0 = ms_vertex(ix, b, c0 + side), q1 = ms_vertex(ix, b, c0 + side + u1);
        const int q2 = ms_vertex(ix, b, c0 + side + u2), q3 = ms_vertex(ix, b, c0 + side + u1 + u2);
        // (q0, q1, q3), (q0, q3, q2) points out of the region for +z, -y, +x when (x, y, z) is right-handed
        const bool straight = (k == 1 || k == 2 || k == 5) != (flip != 0);
        const int b1 = straight ? q1 : q3, c1 = straight ? q3 : q1, b2 = straight ? q3 : q2, c2 = straight ? q2 : q3;
        const long long t = 2 * face;
        ++face;
        if (t + 1 >= n_tri) continue;
        if (layout) {
            uint4 *rec = (uint4 *)cells + t;
            rec[0] = make_uint4(ms_word(3u, 1), ms_word((unsigned int)q0, 1), ms_word((unsigned int)b1, 1), ms_word((unsigned int)c1, 1));
            rec[1] = make_uint4(ms_word(3u, 1), ms_word((unsigned int)q0, 1), ms_word((unsigned int)b2, 1), ms_word((unsigned int)c2, 1));
        } else {
            unsigned int *rec = cells + 3 * t;
            rec[0] = (unsigned int)q0; rec[1] = (unsigned int)b1; rec[2] = (unsigned int)c1;
            rec[3] = (unsigned int)q0; rec[4] = (unsigned int)b2; rec[5] = (unsigned int)c2;
        }
        cell_region[t] = reg;
        cell_region[t + 1] = reg;
    }
}

// ---- host
struct MSCall {
    const char *who;
    const void *seg;
    int label_dtype, n_regions;
    int Z = 0, Y = 0, X = 0;
    long long n_vox = 0;
    int n_tab = 0, W = 1;
    std::vector<unsigned long long> bits;
};

// what the count leaves on the device for the emit: the bits table, the regions with faces, the vertex index
struct MSWork {
    DevBuf table, regs, index;
    std::vector<MSRegion> act;
    MSGeom g{};
    long long cblk = 0, vblk = 0;          // blocks of box corners and of box voxels over all regions
    size_t off_words = 0, off_wpre = 0, off_bcnt = 0, off_fcnt = 0;
    const MSRegion *dregs() const { return regs.as<MSRegion>(); }
    MSIndex ix() const { return MSIndex{index.as<unsigned long long>(off_words), index.as<unsigned int>(off_wpre), index.as<unsigned int>(off_bcnt)}; }
};

// the refusals both entries share, before anything touches the device; *empty: a volume without voxels
int ms_prologue(MSCall &c, const int64_t shape[3], const uint8_t *member, int n_table, std::initializer_list<const void *> host_args, bool *empty) {
    *empty = false;
    bool null_arg = !shape || !member;
    for (const void *p : host_args) null_arg = null_arg || !p;
    if (null_arg) return fnn_failf(FNN_E_INVALID, "%s: NULL argument", c.who);
    if (int rc = fnn_check_label_dtype(c.label_dtype)) return rc;
    if (c.n_regions < 1 || c.n_regions > MS_MAX_REGIONS) return fnn_failf(FNN_E_INVALID, "%s: n_regions must be 1..%d", c.who, MS_MAX_REGIONS);
    if (n_table < 0) return fnn_failf(FNN_E_INVALID, "%s: negative n_table", c.who);
    if (shape[0] < 0 || shape[1] < 0 || shape[2] < 0) return fnn_failf(FNN_E_INVALID, "%s: negative extent", c.who);
    if (shape[0] == 0 || shape[1] == 0 || shape[2] == 0) { *empty = true; return FNN_OK; }
    if (shape[0] > INT_MAX || shape[1] > INT_MAX || shape[2] > INT_MAX || shape[0] * shape[1] > INT_MAX || shape[0] * shape[1] * shape[2] > INT_MAX)
        return fnn_failf(FNN_E_UNSUPPORTED, "%s: more than 2^31 - 1 voxels", c.who);
    c.Z = (int)shape[0]; c.Y = (int)shape[1]; c.X = (int)shape[2];
    c.n_vox = (long long)shape[0] * shape[1] * shape[2];
    return FNN_OK;
}

// bits[v]: one bit per region; values the dtype cannot hold and trailing values of no region are dropped
void ms_table(MSCall &c, const uint8_t *member, int n_table) {
    const int max_value = c.label_dtype == FNN_LABEL_U16 ? 65535 : 255;
    int n_tab = n_table < max_value + 1 ? n_table : max_value + 1;
    auto in_any = [&](int v) {
        for (int r = 0; r < c.n_regions; ++r) if (member[(size_t)r * n_table + v]) return true;
        return false;
    };
    while (n_tab > 0 && !in_any(n_tab - 1)) --n_tab;
    c.n_tab = n_tab;
    c.W = (c.n_regions + 63) / 64;
    c.bits.assign((size_t)(n_tab > 0 ? n_tab : 1) * c.W, 0ull);
    for (int r = 0; r < c.n_regions; ++r)
        for (int v = 0; v < n_tab; ++v)
            if (member[(size_t)r * n_table + v]) c.bits[(size_t)v * c.W + (r >> 6)] |= 1ull << (r & 63);
}

// faces and boxes (one pass over the map), then the corner bits and vertex counts of the regions with faces.  counts
// [n_regions][2] and boxes [n_regions][6] on the host, zeroed by the caller; the stream is synchronised
int ms_count(const MSCall &c, HipCall &call, MSWork &k, int64_t *counts, int64_t *boxes) {
    const size_t R = (size_t)c.n_regions;
    // one block: faces u64 [R] | lo/hi int [R][6] | bits
    const size_t off_box = R * 8, off_bits = (off_box + R * 24 + 7) & ~(size_t)7, n_bits = c.bits.size() * 8;
    if (!k.table.alloc(off_bits + n_bits)) return fnn_failf(FNN_E_HIP, "hipMalloc failed (%s)", c.who);
    std::vector<int> box0(R * 6);
    for (size_t i = 0; i < R * 6; ++i) box0[i] = (i % 6) < 3 ? INT_MAX : -1;
    call.fill(k.table.p, 0, off_box);
    call.copy(k.table.as<char>(off_box), box0.data(), R * 24, hipMemcpyHostToDevice);
    call.copy(k.table.as<char>(off_bits), c.bits.data(), n_bits, hipMemcpyHostToDevice);
    MSGeom &g = k.g;
    g.Z = c.Z; g.Y = c.Y; g.X = c.X;
    g.bits = k.table.as<unsigned long long>(off_bits);
    g.n_tab = c.n_tab;
    g.W = c.W;
    if (c.n_tab == 0) return call.finish();                          // no value of the dtype belongs to a region
    int dev = 0, cus = 0;
    if (call.ok()) call.r = hipGetDevice(&dev);
    if (call.ok()) call.r = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    long long blocks = (c.n_vox + MS_THREADS - 1) / MS_THREADS;
    const long long resident = 8ll * (cus > 0 ? cus : 1);
    if (blocks > resident) blocks = resident;
    fnn_by_label(c.label_dtype, [&](auto lt) {
        using T = decltype(lt);
        call.launch(ms_count_kernel<T>, dim3((unsigned)blocks), dim3(MS_THREADS), R * 32, (const T *)c.seg, g, c.n_regions,
                    k.table.as<unsigned long long>(), k.table.as<int>(off_box));
    });
    std::vector<unsigned long long> hcnt(R);
    std::vector<int> hbox(R * 6);
    call.copy(hcnt.data(), k.table.p, R * 8, hipMemcpyDeviceToHost);
    call.copy(hbox.data(), k.table.as<char>(off_box), R * 24, hipMemcpyDeviceToHost);
    if (!call.sync()) return call.fail();
    for (size_t r = 0; r < R; ++r) {
        if (!hcnt[r]) continue;
        counts[2 * r + 1] = (int64_t)hcnt[r];
        const int *b = hbox.data() + 6 * r;
        for (int a = 0; a < 3; ++a) { boxes[6 * r + 2 * a] = b[a]; boxes[6 * r + 2 * a + 1] = b[3 + a] + 1; }
        MSRegion m{b[0], b[1], b[2], b[3] + 1 - b[0], b[4] + 1 - b[1], b[5] + 1 - b[2], (int)r, 0u, 0u};
        const long long n_c = (long long)(m.bz + 1) * (m.by + 1) * (m.bx + 1), n_box = (long long)m.bz * m.by * m.bx;
        if (k.cblk > INT_MAX || k.vblk > INT_MAX) break;
        m.cblk0 = (unsigned int)k.cblk;
        m.vblk0 = (unsigned int)k.vblk;
        k.cblk += (n_c + MS_BLOCK - 1) / MS_BLOCK;
        k.vblk += (n_box + MS_BLOCK - 1) / MS_BLOCK;
        k.act.push_back(m);
    }
    if (k.act.empty()) return FNN_OK;
    if (k.cblk > INT_MAX || k.vblk > INT_MAX) return fnn_failf(FNN_E_UNSUPPORTED, "%s: the boxes of the regions hold more than 2^41 corners", c.who);
    // vertices u64 [regions with faces] | words u64 [cblk][16] | word prefixes u32 [cblk][16] | block counts u32 [cblk] | face counts u32 [vblk]
    const size_t A = k.act.size();
    k.off_words = A * 8;
    k.off_wpre = k.off_words + (size_t)k.cblk * MS_WORDS * 8;
    k.off_bcnt = k.off_wpre + (size_t)k.cblk * MS_WORDS * 4;
    k.off_fcnt = k.off_bcnt + (size_t)k.cblk * 4;
    if (!k.regs.alloc(A * sizeof(MSRegion)) || !k.index.alloc(k.off_fcnt + (size_t)k.vblk * 4))
        return fnn_failf(FNN_E_HIP, "hipMalloc failed (%s: 196 B per 1024 box corners and 4 B per 1024 box voxels of scratch)", c.who);
    call.copy(k.regs.p, k.act.data(), A * sizeof(MSRegion), hipMemcpyHostToDevice);
    call.fill(k.index.p, 0, A * 8);
    fnn_by_label(c.label_dtype, [&](auto lt) {
        using T = decltype(lt);
        call.launch(ms_corner_kernel<T>, dim3((unsigned)k.cblk), dim3(MS_BLOCK), 0, (const T *)c.seg, g, k.dregs(), (int)A,
                    k.index.as<unsigned long long>(k.off_words), k.index.as<unsigned int>(k.off_wpre), k.index.as<unsigned int>(k.off_bcnt),
                    k.index.as<unsigned long long>());
    });
    std::vector<unsigned long long> hv(A);
    call.copy(hv.data(), k.index.p, A * 8, hipMemcpyDeviceToHost);
    if (!call.sync()) return call.fail();
    for (size_t a = 0; a < A; ++a) counts[2 * k.act[a].r] = (int64_t)hv[a];
    return FNN_OK;
}

}  // namespace

extern "C" {

int fnn_mesh_count(const void *seg, int label_dtype, const int64_t shape[3], const uint8_t *member, int n_table, int n_regions,
                   int64_t *counts, int64_t *boxes, void *stream) {
    MSCall c{"fnn_mesh_count", seg, label_dtype, n_regions};
    bool empty;
    if (int rc = ms_prologue(c, shape, member, n_table, {counts, boxes}, &empty)) return rc;
    for (int k = 0; k < n_regions * 2; ++k) counts[k] = 0;
    for (int k = 0; k < n_regions * 6; ++k) boxes[k] = 0;
    if (empty) return FNN_OK;
    if (seg && label_dtype == FNN_LABEL_U16 && ((uintptr_t)seg & 1)) return fnn_failf(FNN_E_INVALID, "%s: the label map must be aligned to its element", c.who);
    if (int rc = fnn_need_dev(c.who, {seg}, "a device label map")) return rc;
    ms_table(c, member, n_table);
    HipCall call(stream);
    MSWork k;
    return ms_count(c, call, k, counts, boxes);
}

int fnn_mesh_emit(const void *seg, int label_dtype, const int64_t shape[3], const uint8_t *member, int n_table, int n_regions,
                  const double affine[16], int smoothing_pairs, int layout, void *points, int64_t cap_points, void *cells, int64_t cap_cells,
                  void *cell_region, void *stream) {
    MSCall c{"fnn_mesh_emit", seg, label_dtype, n_regions};
    bool empty;
    if (int rc = ms_prologue(c, shape, member, n_table, {affine}, &empty)) return rc;
    for (int k = 0; k < 16; ++k)
        if (!std::isfinite(affine[k])) return fnn_failf(FNN_E_INVALID, "%s: the affine must be finite", c.who);
    if (smoothing_pairs < 0) return fnn_failf(FNN_E_INVALID, "%s: smoothing_pairs is negative", c.who);
    if (layout != 0 && layout != 1) return fnn_failf(FNN_E_INVALID, "%s: unknown layout", c.who);
    if (cap_points < 0 || cap_cells < 0) return fnn_failf(FNN_E_INVALID, "%s: a cap is negative", c.who);
    if (empty) return FNN_OK;
    if (seg && label_dtype == FNN_LABEL_U16 && ((uintptr_t)seg & 1)) return fnn_failf(FNN_E_INVALID, "%s: the label map must be aligned to its element", c.who);
    if (((uintptr_t)points & 3) || ((uintptr_t)cells & (layout ? 15 : 3)) || ((uintptr_t)cell_region & 1))
        return fnn_failf(FNN_E_INVALID, "%s: points must be 4-byte, cells %d-byte and cell_region 2-byte aligned", c.who, layout ? 16 : 4);
    if (int rc = fnn_need_dev(c.who, {seg, points, cells, cell_region}, "device pointers for seg, points, cells and cell_region")) return rc;
    ms_table(c, member, n_table);
    HipCall call(stream);
    MSWork k;
    std::vector<int64_t> counts((size_t)n_regions * 2, 0), boxes((size_t)n_regions * 6, 0);
    if (int rc = ms_count(c, call, k, counts.data(), boxes.data())) return rc;
    long long n = 0, faces = 0;
    for (int r = 0; r < n_regions; ++r) { n += counts[2 * r]; faces += counts[2 * r + 1]; }
    if (n > INT_MAX) return fnn_failf(FNN_E_UNSUPPORTED, "%s: more than 2^31 - 1 vertices", c.who);
    if (2 * faces > INT_MAX) return fnn_failf(FNN_E_UNSUPPORTED, "%s: more than 2^31 - 1 triangles", c.who);
    if (cap_points < n) return fnn_failf(FNN_E_INVALID, "%s: cap_points is below the number of points (%lld)", c.who, n);
    if (cap_cells < 2 * faces) return fnn_failf(FNN_E_INVALID, "%s: cap_cells is below the number of triangles (%lld)", c.who, 2 * faces);
    if (faces == 0) return FNN_OK;

    // positions f32 [n][3], twice and the neighbours i32 [6][n] when there is smoothing
    const size_t pos_bytes = (size_t)n * 12;
    DevBuf work;
    if (!work.alloc(smoothing_pairs ? pos_bytes * 4 : pos_bytes)) return fnn_failf(FNN_E_HIP, "hipMalloc failed (%s: 12 B per vertex, 48 B with smoothing)", c.who);
    float *pos = work.as<float>(), *other = smoothing_pairs ? work.as<float>(pos_bytes) : nullptr;
    int *nbr = smoothing_pairs ? work.as<int>(2 * pos_bytes) : nullptr;
    MSAffine A;
    for (int r = 0; r < 3; ++r)
        for (int j = 0; j < 4; ++j) A.a[r][j] = affine[4 * r + j];
    const double det = A.a[0][0] * (A.a[1][1] * A.a[2][2] - A.a[1][2] * A.a[2][1]) - A.a[0][1] * (A.a[1][0] * A.a[2][2] - A.a[1][2] * A.a[2][0]) +
                       A.a[0][2] * (A.a[1][0] * A.a[2][1] - A.a[1][1] * A.a[2][0]);
    const int n_act = (int)k.act.size();
    const MSIndex ix = k.ix();
    unsigned int *bcnt = k.index.as<unsigned int>(k.off_bcnt), *fcnt = k.index.as<unsigned int>(k.off_fcnt);
    const unsigned vgrid = (unsigned)((n + MS_THREADS - 1) / MS_THREADS);
    fnn_by_label(label_dtype, [&](auto lt) {
        using T = decltype(lt);
        const T *s = (const T *)seg;
        call.launch(ms_scan_kernel, dim3(1), dim3(MS_BLOCK), 0, bcnt, (int)k.cblk);
        call.launch(ms_face_count_kernel<T>, dim3((unsigned)k.vblk), dim3(MS_BLOCK), 0, s, k.g, k.dregs(), n_act, fcnt);
        call.launch(ms_scan_kernel, dim3(1), dim3(MS_BLOCK), 0, fcnt, (int)k.vblk);
        call.launch(ms_points_kernel<T>, dim3((unsigned)k.cblk), dim3(MS_BLOCK), 0, s, k.g, k.dregs(), n_act, ix, pos, nbr, n);
        for (int p = 0; p < smoothing_pairs; ++p) {
            call.launch(ms_smooth_kernel, dim3(vgrid), dim3(MS_THREADS), 0, (const float *)pos, (const int *)nbr, n, 0.5f, other);
            call.launch(ms_smooth_kernel, dim3(vgrid), dim3(MS_THREADS), 0, (const float *)other, (const int *)nbr, n, -0.53f, pos);
        }
        call.launch(ms_world_kernel, dim3(vgrid), dim3(MS_THREADS), 0, (const float *)pos, n, A, layout, (unsigned int *)points);
        call.launch(ms_cells_kernel<T>, dim3((unsigned)k.vblk), dim3(MS_BLOCK), 0, s, k.g, k.dregs(), n_act, ix, (const unsigned int *)fcnt,
                    det < 0.0 ? 1 : 0, layout, (unsigned int *)cells, (unsigned short *)cell_region, 2 * faces);
    });
    return call.finish();
}

}  // extern "C"
