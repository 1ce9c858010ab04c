// surface.hip - exact surface distances between two label maps for HD / HD95 / ASSD / NSD, gfx950.
//
//   fnn_surface_count       per region: the surface voxels of the reference and of the prediction and the [lo, hi) box of both
//   fnn_surface_distances   per region: the squared distances d(pred -> ref), then d(ref -> pred), compacted in raster order
//
// The surface of a mask is the mask minus its 6-neighbourhood erosion, everything outside the volume being background.  A
// region is a set of label values; bits[v] holds one bit per region that value v belongs to, so one pass over both maps
// finds the surface voxels of every region at once: bits[centre] & ~(AND of bits[six neighbours]).  The extremes of a mask
// are surface voxels, so the box of the surfaces is the box of the masks.
//
// The distance transform of one region and direction runs inside the region's box, separable in the order z, y, x:
//   z   one thread per column: a sweep that fills the gaps between surface voxels with the voxel count |dz| to the nearer
//       one (int32, -1: none in the column);
//   y   out[i] = min over q of ((sz dz[q])^2 + (sy (i - q))^2), every value evaluated in float64 as written; a tile of
//       128 x 32 line elements is staged in LDS and each output walks outward from i, q = i -+ k, until (sy k)^2 is not
//       below the best value so far - that term only grows, so the stop is exact.  Elements of the line outside the tile are
//       read from global memory;
//   x   the same walk along x, only for the surface voxels of the other mask, fused with the ordered compaction: a block
//       owns 1024 raster-consecutive box voxels (staged in LDS), and its surface voxels are written at the block's offset
//       (an exclusive scan of per-block counts) plus their rank in the block (ballots).
// No floating-point atomics and no atomic counters in the compaction: the same input gives the same bytes.
// The sums must not be contracted into fused multiply-adds - the yardstick's values are products rounded, then added.
#pragma clang fp contract(off)
#include "host_call.h"
#include <climits>
#include <cmath>
#include <vector>

namespace {

constexpr int SF_THREADS = 256;
constexpr int SF_MAX_REGIONS = 1024;       // 8 LDS words per region in the count kernel: 32 KiB
constexpr int SF_PIECE = 1024;             // raster-consecutive box voxels per block of the x pass (its line tile)
constexpr int SF_YT_X = 32, SF_YT_Y = 128; // the y pass stages 128 line elements of 32 adjacent lines: 32 KiB

struct SFGeom {
    int Z, Y, X;
    const unsigned long long *bits;        // [n_tab][W]: bit r of bits[v] - value v belongs to region r
    int n_tab, W;
};
struct SFBox { int z0, y0, x0, bz, by, bx; };

__device__ __forceinline__ unsigned long long sf_bits(const SFGeom &g, int v, int w) {
    return v < g.n_tab ? g.bits[(size_t)v * g.W + w] : 0ull;
}
__device__ __forceinline__ bool sf_member(const SFGeom &g, int r, int v) { return (sf_bits(g, v, r >> 6) >> (r & 63)) & 1ull; }

// is voxel (z, y, x) of the volume a surface voxel of region r in map m?
template <typename T>
__device__ __forceinline__ bool sf_surface(const T *m, const SFGeom &g, int r, int z, int y, int x) {
    const size_t i = ((size_t)z * g.Y + y) * g.X + x;
    const int v = m[i];
    if (!sf_member(g, r, v)) return false;
    if (z == 0 || y == 0 || x == 0 || z == g.Z - 1 || y == g.Y - 1 || x == g.X - 1) return true;
    const size_t sy = (size_t)g.X, sz = (size_t)g.Y * g.X;
    const int a = m[i - 1], b = m[i + 1], c = m[i - sy], d = m[i + sy], e = m[i - sz], f = m[i + sz];
    if (a == v && b == v && c == v && d == v && e == v && f == v) return false;
    return !(sf_member(g, r, a) && sf_member(g, r, b) && sf_member(g, r, c) && sf_member(g, r, d) && sf_member(g, r, e) &&
             sf_member(g, r, f));
}

// ---- surface sizes and boxes of every region, one pass over both maps
// LDS: [n_regions][8] = surface voxels of ref, of pred, lowest z, y, x, highest z, y, x.  Only surface voxels touch it (LDS
// integer atomics), and a block adds to the global words once per region it met.
template <typename T>
__global__ __launch_bounds__(SF_THREADS) void sf_count_kernel(const T *ref, const T *pred, SFGeom g, int n_regions,
                                                               unsigned long long *gcnt, int *gbox) {
    extern __shared__ int acc[];
    for (int k = threadIdx.x; k < n_regions * 8; k += SF_THREADS) acc[k] = (k & 7) < 2 ? 0 : ((k & 7) < 5 ? INT_MAX : -1);
    __syncthreads();
    const long long n = (long long)g.Z * g.Y * g.X, stride = (long long)gridDim.x * SF_THREADS;
    const int plane = g.Y * g.X;
    for (long long i = (long long)blockIdx.x * SF_THREADS + threadIdx.x; i < n; i += stride) {
        const int z = (int)(i / plane), rem = (int)(i - (long long)z * plane), y = rem / g.X, x = rem - y * g.X;
        const bool face = z == 0 || y == 0 || x == 0 || z == g.Z - 1 || y == g.Y - 1 || x == g.X - 1;
#pragma unroll
        for (int side = 0; side < 2; ++side) {
            const T *m = side ? pred : ref;
            const int v = m[i];
            if (v >= g.n_tab) continue;
            int a = 0, b = 0, c = 0, d = 0, e = 0, f = 0;
            if (!face) {
                a = m[i - 1]; b = m[i + 1]; c = m[i - g.X]; d = m[i + g.X]; e = m[i - plane]; f = m[i + plane];
                if (a == v && b == v && c == v && d == v && e == v && f == v) continue;
            }
            for (int w = 0; w < g.W; ++w) {
                const unsigned long long in = g.bits[(size_t)v * g.W + w];
                if (!in) continue;
                const unsigned long long around = face ? 0ull : (sf_bits(g, a, w) & sf_bits(g, b, w) & sf_bits(g, c, w) &
                                                                 sf_bits(g, d, w) & sf_bits(g, e, w) & sf_bits(g, f, w));
                unsigned long long s = in & ~around;
                while (s) {
                    const int r = w * 64 + __ffsll((long long)s) - 1;
                    s &= s - 1;
                    int *q = acc + r * 8;
                    atomicAdd(q + side, 1);
                    atomicMin(q + 2, z); atomicMin(q + 3, y); atomicMin(q + 4, x);
                    atomicMax(q + 5, z); atomicMax(q + 6, y); atomicMax(q + 7, x);
                }
            }
        }
    }
    __syncthreads();
    for (int r = threadIdx.x; r < n_regions; r += SF_THREADS) {
        const int *q = acc + r * 8;
        if (q[0] == 0 && q[1] == 0) continue;
        if (q[0]) atomicAdd(gcnt + 2 * r, (unsigned long long)q[0]);
        if (q[1]) atomicAdd(gcnt + 2 * r + 1, (unsigned long long)q[1]);
        for (int k = 0; k < 3; ++k) { atomicMin(gbox + 6 * r + k, q[2 + k]); atomicMax(gbox + 6 * r + 3 + k, q[5 + k]); }
    }
}

// ---- z pass: per column of the box the voxel count to the nearest surface voxel of region r in map m, -1 without one
template <typename T>
__global__ __launch_bounds__(SF_THREADS) void sf_zpass_kernel(const T *m, SFGeom g, SFBox b, int r, int *dz) {
    const long long col = (long long)blockIdx.x * SF_THREADS + threadIdx.x;
    const size_t plane = (size_t)b.by * b.bx;
    if (col >= (long long)plane) return;
    const int y = (int)(col / b.bx), x = (int)(col - (long long)y * b.bx);
    int last = -1;
    for (int z = 0; z < b.bz; ++z) {
        if (!sf_surface<T>(m, g, r, b.z0 + z, b.y0 + y, b.x0 + x)) continue;
        for (int zz = last + 1; zz < z; ++zz) {
            int d = z - zz;
            if (last >= 0 && zz - last < d) d = zz - last;
            dz[(size_t)zz * plane + col] = d;
        }
        dz[(size_t)z * plane + col] = 0;
        last = z;
    }
    for (int zz = last + 1; zz < b.bz; ++zz) dz[(size_t)zz * plane + col] = last < 0 ? -1 : zz - last;
}

__device__ __forceinline__ double sf_sq(double s, int k) {
    const double d = s * (double)k;
    return d * d;
}
__device__ __forceinline__ double sf_g0(double sz, int d) { return d < 0 ? (double)INFINITY : sf_sq(sz, d); }

// ---- y pass: out[z][y][x] = min over q of ((sz dz[z][q][x])^2 + (sy (y - q))^2)
__global__ __launch_bounds__(SF_THREADS) void sf_ypass_kernel(const int *dz, SFBox b, double sz, double sy, double *out) {
    __shared__ double tile[SF_YT_Y][SF_YT_X];
    const int tiles_x = (b.bx + SF_YT_X - 1) / SF_YT_X, tiles_y = (b.by + SF_YT_Y - 1) / SF_YT_Y;
    const int tx = blockIdx.x % tiles_x, ty = (blockIdx.x / tiles_x) % tiles_y, z = blockIdx.x / (tiles_x * tiles_y);
    const int lx = threadIdx.x & (SF_YT_X - 1), ly = threadIdx.x / SF_YT_X;
    const int x = tx * SF_YT_X + lx, y0 = ty * SF_YT_Y;
    const int *line = dz + (size_t)z * b.by * b.bx + x;             // element q of the line: line[q * bx]
    if (x < b.bx)
        for (int yy = ly; yy < SF_YT_Y && y0 + yy < b.by; yy += SF_THREADS / SF_YT_X)
            tile[yy][lx] = sf_g0(sz, line[(size_t)(y0 + yy) * b.bx]);
    __syncthreads();
    if (x >= b.bx) return;
    for (int yy = ly; yy < SF_YT_Y && y0 + yy < b.by; yy += SF_THREADS / SF_YT_X) {
        const int y = y0 + yy;
        double best = tile[yy][lx];
        for (int k = 1;; ++k) {
            const double t = sf_sq(sy, k);
            if (!(t < best)) break;
            const int lo = y - k, hi = y + k;
            if (lo < 0 && hi >= b.by) break;
            if (lo >= 0) {
                const double c = (lo >= y0 ? tile[lo - y0][lx] : sf_g0(sz, line[(size_t)lo * b.bx])) + t;
                if (c < best) best = c;
            }
            if (hi < b.by) {
                const double c = (hi < y0 + SF_YT_Y ? tile[hi - y0][lx] : sf_g0(sz, line[(size_t)hi * b.bx])) + t;
                if (c < best) best = c;
            }
        }
        out[((size_t)z * b.by + y) * b.bx + x] = best;
    }
}

// voxel i of the box in raster order -> is it a surface voxel of region r in map m
template <typename T>
__device__ __forceinline__ bool sf_box_surface(const T *m, const SFGeom &g, const SFBox &b, int r, long long i, int &x) {
    const long long plane = (long long)b.by * b.bx;
    const int z = (int)(i / plane), rem = (int)(i - z * plane), y = rem / b.bx;
    x = rem - y * b.bx;
    return sf_surface<T>(m, g, r, b.z0 + z, b.y0 + y, b.x0 + x);
}

// ---- surface voxels per block of SF_PIECE raster-consecutive box voxels
template <typename T>
__global__ __launch_bounds__(SF_PIECE) void sf_piece_count_kernel(const T *m, SFGeom g, SFBox b, int r, long long n_box, unsigned int *counts) {
    __shared__ unsigned int wave_n[SF_PIECE / 64];
    const long long i = (long long)blockIdx.x * SF_PIECE + threadIdx.x;
    int x;
    const bool s = i < n_box && sf_box_surface<T>(m, g, b, r, i, x);
    const unsigned long long vote = __ballot(s);
    if ((threadIdx.x & 63) == 0) wave_n[threadIdx.x >> 6] = (unsigned int)__popcll(vote);
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned int t = 0;
        for (int k = 0; k < SF_PIECE / 64; ++k) t += wave_n[k];
        counts[blockIdx.x] = t;
    }
}

// ---- exclusive scan of the per-block counts in place, one block
__global__ __launch_bounds__(SF_PIECE) void sf_scan_kernel(unsigned int *counts, int n) {
    __shared__ unsigned int wave_sum[SF_PIECE / 64];
    __shared__ unsigned int carry;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (int base = 0; base < n; base += SF_PIECE) {
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
        if (threadIdx.x == SF_PIECE - 1) carry = before + v;
        __syncthreads();
    }
}

// ---- x pass at the surface voxels of region r in map m, written compacted in raster order:
// dst[offsets[block] + rank in block] = min over q of (gy[line][q] + (sx (x - q))^2)
template <typename T>
__global__ __launch_bounds__(SF_PIECE) void sf_gather_kernel(const T *m, SFGeom g, SFBox b, int r, long long n_box, const double *gy,
                                                              double sx, const unsigned int *offsets, double *dst, long long n_dst) {
    __shared__ double tile[SF_PIECE];
    __shared__ unsigned int wave_n[SF_PIECE / 64];
    const long long b0 = (long long)blockIdx.x * SF_PIECE, i = b0 + threadIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int x = 0;
    const bool s = i < n_box && sf_box_surface<T>(m, g, b, r, i, x);
    if (i < n_box) tile[threadIdx.x] = gy[i];
    const unsigned long long vote = __ballot(s);
    if (lane == 0) wave_n[wave] = (unsigned int)__popcll(vote);
    __syncthreads();
    if (!s) return;
    long long at = (long long)offsets[blockIdx.x] + __popcll(vote & ((1ull << lane) - 1ull));
    for (int k = 0; k < wave; ++k) at += wave_n[k];
    double best = tile[threadIdx.x];
    const long long b1 = b0 + SF_PIECE;
    for (int k = 1;; ++k) {
        const double t = sf_sq(sx, k);
        if (!(t < best)) break;
        const int lo = x - k, hi = x + k;
        if (lo < 0 && hi >= b.bx) break;
        if (lo >= 0) {
            const double c = (i - k >= b0 ? tile[threadIdx.x - k] : gy[i - k]) + t;
            if (c < best) best = c;
        }
        if (hi < b.bx) {
            const double c = (i + k < b1 ? tile[threadIdx.x + k] : gy[i + k]) + t;
            if (c < best) best = c;
        }
    }
    if (at < n_dst) dst[at] = best;
}

// ---- host
struct SFCall {
    const char *who;
    const void *ref, *pred;
    int label_dtype, n_regions;
    int Z = 0, Y = 0, X = 0;
    long long n_vox = 0;
    int n_tab = 0, W = 1;
    std::vector<unsigned long long> bits;
};

// the refusals both entries share, before anything touches the device; *empty: a volume without voxels.  host_args: the
// entry's host pointers besides shape and member; with_spacing: the distances entry, which also has spacing, out and cap
int sf_prologue(SFCall &c, const int64_t shape[3], const uint8_t *member, int n_table, std::initializer_list<const void *> host_args,
                bool with_spacing, const double *spacing, const void *out, long long cap, bool *empty) {
    *empty = false;
    bool null_arg = !shape || !member;
    for (const void *p : host_args) null_arg = null_arg || !p;
    if (null_arg) return fnn_failf(FNN_E_INVALID, "%s: NULL argument", c.who);
    if (int rc = fnn_check_label_dtype(c.label_dtype)) return rc;
    if (c.n_regions < 1 || c.n_regions > SF_MAX_REGIONS) return fnn_failf(FNN_E_INVALID, "%s: n_regions must be 1..%d", c.who, SF_MAX_REGIONS);
    if (n_table < 0) return fnn_failf(FNN_E_INVALID, "%s: negative n_table", c.who);
    if (shape[0] < 0 || shape[1] < 0 || shape[2] < 0) return fnn_failf(FNN_E_INVALID, "%s: negative extent", c.who);
    if (with_spacing) {
        for (int k = 0; k < 3; ++k)
            if (!(spacing[k] > 0.0) || !std::isfinite(spacing[k])) return fnn_failf(FNN_E_INVALID, "%s: spacing must be finite and positive", c.who);
        if (cap < 0) return fnn_failf(FNN_E_INVALID, "%s: cap is negative", c.who);
    }
    if (shape[0] == 0 || shape[1] == 0 || shape[2] == 0) { *empty = true; return FNN_OK; }
    if (shape[0] > INT_MAX || shape[1] > INT_MAX || shape[2] > INT_MAX || shape[0] * shape[1] > INT_MAX ||
        shape[0] * shape[1] * shape[2] > INT_MAX)
        return fnn_failf(FNN_E_UNSUPPORTED, "%s: more than 2^31 - 1 voxels", c.who);
    const uintptr_t emask = c.label_dtype == FNN_LABEL_U16 ? 1 : 0;
    if (c.ref && c.pred && (((uintptr_t)c.ref | (uintptr_t)c.pred) & emask)) return fnn_failf(FNN_E_INVALID, "%s: label maps must be aligned to their element", c.who);
    if (with_spacing && out && ((uintptr_t)out & 7)) return fnn_failf(FNN_E_INVALID, "%s: sq_dist must be 8-byte aligned", c.who);
    if (with_spacing) {
        if (int rc = fnn_need_dev(c.who, {c.ref, c.pred, out}, "device pointers for ref, pred and sq_dist")) return rc;
    } else if (int rc = fnn_need_dev(c.who, {c.ref, c.pred}, "device label maps")) return rc;
    c.Z = (int)shape[0]; c.Y = (int)shape[1]; c.X = (int)shape[2];
    c.n_vox = (long long)shape[0] * shape[1] * shape[2];
    // bits[v]: one bit per region; values the dtype cannot hold and trailing values of no region are dropped
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
    return FNN_OK;
}

// the count pass: n_surface [n_regions][2] and boxes [n_regions][6] on the host, the bits table left on the device
int sf_count(const SFCall &c, HipCall &call, DevBuf &table, SFGeom &g, int64_t *n_surface, int64_t *boxes) {
    const size_t R = (size_t)c.n_regions;
    // one block: counts u64 [R][2] | lo/hi int [R][6] | bits
    const size_t off_box = R * 16, off_bits = (off_box + R * 24 + 7) & ~(size_t)7, n_bits = c.bits.size() * 8;
    if (!table.alloc(off_bits + n_bits)) return fnn_failf(FNN_E_HIP, "hipMalloc failed (%s)", c.who);
    std::vector<int> box0(R * 6);
    for (size_t k = 0; k < R * 6; ++k) box0[k] = (k % 6) < 3 ? INT_MAX : -1;
    call.fill(table.p, 0, off_box);
    call.copy(table.as<char>(off_box), box0.data(), R * 24, hipMemcpyHostToDevice);
    call.copy(table.as<char>(off_bits), c.bits.data(), n_bits, hipMemcpyHostToDevice);
    g.Z = c.Z; g.Y = c.Y; g.X = c.X;
    g.bits = table.as<unsigned long long>(off_bits);
    g.n_tab = c.n_tab;
    g.W = c.W;
    int dev = 0, cus = 0;
    if (call.ok()) call.r = hipGetDevice(&dev);
    if (call.ok()) call.r = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    long long blocks = (c.n_vox + SF_THREADS - 1) / SF_THREADS;
    const long long resident = 8ll * (cus > 0 ? cus : 1);
    if (blocks > resident) blocks = resident;
    if (c.n_tab > 0)
        fnn_by_label(c.label_dtype, [&](auto lt) {
            using T = decltype(lt);
            call.launch(sf_count_kernel<T>, dim3((unsigned)blocks), dim3(SF_THREADS), R * 32, (const T *)c.ref, (const T *)c.pred, g,
                        c.n_regions, table.as<unsigned long long>(), table.as<int>(off_box));
        });
    std::vector<unsigned long long> hcnt(R * 2);
    std::vector<int> hbox(R * 6);
    call.copy(hcnt.data(), table.p, R * 16, hipMemcpyDeviceToHost);
    call.copy(hbox.data(), table.as<char>(off_box), R * 24, hipMemcpyDeviceToHost);
    if (!call.sync()) return call.fail();
    for (size_t r = 0; r < R; ++r) {
        n_surface[2 * r] = (int64_t)hcnt[2 * r];
        n_surface[2 * r + 1] = (int64_t)hcnt[2 * r + 1];
        const bool none = hcnt[2 * r] == 0 && hcnt[2 * r + 1] == 0;
        for (int k = 0; k < 3; ++k) {
            boxes[6 * r + 2 * k] = none ? 0 : hbox[6 * r + k];
            boxes[6 * r + 2 * k + 1] = none ? 0 : hbox[6 * r + 3 + k] + 1;
        }
    }
    return FNN_OK;
}

}  // namespace

extern "C" {

int fnn_surface_count(const void *ref, const void *pred, int label_dtype, const int64_t shape[3], const uint8_t *member, int n_table,
                      int n_regions, int64_t *n_surface, int64_t *boxes, void *stream) {
    SFCall c{"fnn_surface_count", ref, pred, label_dtype, n_regions};
    bool empty;
    if (int rc = sf_prologue(c, shape, member, n_table, {n_surface, boxes}, false, nullptr, nullptr, 0, &empty)) return rc;
    for (int k = 0; k < n_regions * 2; ++k) n_surface[k] = 0;
    for (int k = 0; k < n_regions * 6; ++k) boxes[k] = 0;
    if (empty) return FNN_OK;
    HipCall call(stream);
    DevBuf table;
    SFGeom g{};
    return sf_count(c, call, table, g, n_surface, boxes);
}

int fnn_surface_distances(const void *ref, const void *pred, int label_dtype, const int64_t shape[3], const uint8_t *member, int n_table,
                          int n_regions, const double spacing[3], double *sq_dist, int64_t cap, void *stream) {
    SFCall c{"fnn_surface_distances", ref, pred, label_dtype, n_regions};
    bool empty;
    if (int rc = sf_prologue(c, shape, member, n_table, {spacing}, true, spacing, sq_dist, cap, &empty)) return rc;
    if (empty) return FNN_OK;
    HipCall call(stream);
    DevBuf table;
    SFGeom g{};
    std::vector<int64_t> ns((size_t)n_regions * 2), bx((size_t)n_regions * 6);
    if (int rc = sf_count(c, call, table, g, ns.data(), bx.data())) return rc;
    long long total = 0, max_box = 0;
    for (int r = 0; r < n_regions; ++r) {
        if (!ns[2 * r] || !ns[2 * r + 1]) continue;
        total += ns[2 * r] + ns[2 * r + 1];
        const long long v = (bx[6 * r + 1] - bx[6 * r]) * (bx[6 * r + 3] - bx[6 * r + 2]) * (bx[6 * r + 5] - bx[6 * r + 4]);
        if (v > max_box) max_box = v;
    }
    if (cap < total) return fnn_failf(FNN_E_INVALID, "fnn_surface_distances: cap is below the number of distances (%lld)", total);
    if (total == 0) return FNN_OK;

    // workspace: y-pass values f64 [max_box] | z-pass counts i32 [max_box] | per-block counts u32 [pieces]
    const long long pieces_max = (max_box + SF_PIECE - 1) / SF_PIECE;
    const size_t off_dz = (size_t)max_box * 8, off_cnt = (off_dz + (size_t)max_box * 4 + 7) & ~(size_t)7;
    DevBuf work;
    if (!work.alloc(off_cnt + (size_t)pieces_max * 4)) return fnn_fail(FNN_E_HIP, "hipMalloc failed (12 B per box voxel of scratch)");
    double *gy = work.as<double>();
    int *dz = work.as<int>(off_dz);
    unsigned int *counts = work.as<unsigned int>(off_cnt);

    long long at = 0;
    fnn_by_label(label_dtype, [&](auto lt) {
        using T = decltype(lt);
        for (int r = 0; r < n_regions; ++r) {
            if (!ns[2 * r] || !ns[2 * r + 1]) continue;
            SFBox b{(int)bx[6 * r], (int)bx[6 * r + 2], (int)bx[6 * r + 4], (int)(bx[6 * r + 1] - bx[6 * r]),
                    (int)(bx[6 * r + 3] - bx[6 * r + 2]), (int)(bx[6 * r + 5] - bx[6 * r + 4])};
            const long long n_box = (long long)b.bz * b.by * b.bx, cols = (long long)b.by * b.bx;
            const long long pieces = (n_box + SF_PIECE - 1) / SF_PIECE;
            const long long ytiles = (long long)((b.bx + SF_YT_X - 1) / SF_YT_X) * ((b.by + SF_YT_Y - 1) / SF_YT_Y) * b.bz;
            for (int dir = 0; dir < 2; ++dir) {                      // 0: from pred's surface to ref's, 1: the other way
                const T *to = (const T *)(dir ? pred : ref), *from = (const T *)(dir ? ref : pred);
                const long long n_from = ns[2 * r + (dir ? 0 : 1)];
                call.launch(sf_zpass_kernel<T>, dim3((unsigned)((cols + SF_THREADS - 1) / SF_THREADS)), dim3(SF_THREADS), 0, to, g, b, r, dz);
                call.launch(sf_ypass_kernel, dim3((unsigned)ytiles), dim3(SF_THREADS), 0, (const int *)dz, b, spacing[0], spacing[1], gy);
                call.launch(sf_piece_count_kernel<T>, dim3((unsigned)pieces), dim3(SF_PIECE), 0, from, g, b, r, n_box, counts);
                call.launch(sf_scan_kernel, dim3(1), dim3(SF_PIECE), 0, counts, (int)pieces);
                call.launch(sf_gather_kernel<T>, dim3((unsigned)pieces), dim3(SF_PIECE), 0, from, g, b, r, n_box, (const double *)gy,
                            spacing[2], (const unsigned int *)counts, sq_dist + at, n_from);
                at += n_from;
            }
        }
    });
    return call.finish();
}

}  // extern "C"
