// morph.hip - binary morphology of one label set on the label map, gfx950: fnn_binary_morphology (dilate, erode, open, close
// with scipy's generate_binary_structure(ndim, rank), n iterations and a border value).  morph_core.h holds the rule, the
// geometry of the bit planes and why one `outside` bit per call is enough; this file is its loaders and launches:
//   a. box     border_value 0 only: the bounding box of the set S (fill_holes_box_kernel.h, the pass fnn_fill_holes makes),
//              read by the host - an empty S ends the call; the box is grown by n for dilation and closing.  With
//              border_value 1 the box is the whole volume;
//   b. pack    one wave per word: a ballot of table[label] >= 0 over 64 consecutive z-voxels of a row of the box;
//   c. step    n launches per run of the operation (one run for dilate / erode, two for open / close), ping-pong between
//              two planes, one thread per output word; rank and operation are template arguments;
//   d. apply   one wave per word of the final plane: the label rule in place, written voxels counted (one atomic per wave).
// Scratch, allocated inside the call: two planes = 2 bits per voxel of the box (rows padded to whole words).
#include "fill_holes_box_kernel.h"
#include "morph_core.h"
#include <climits>

namespace {

constexpr int MORPH_THREADS = 256;                 // 4 waves
constexpr unsigned MORPH_MAX_BLOCKS = 8192;        // pack / apply walk the words with a grid stride

struct MorphGeom {
    FHBox b;                                       // the box in the volume
    int Y, Z;                                      // the volume's inner extents
    int W;                                         // words per row of the box
    int n_words;                                   // bx * by * W
};

__device__ __forceinline__ int morph_voxel(const MorphGeom &g, int row, int z) {
    const int y = row % g.b.by, x = row / g.b.by;
    return ((g.b.x0 + x) * g.Y + (g.b.y0 + y)) * g.Z + (g.b.z0 + z);
}

// b. labels -> plane.  A wave takes word after word; lane i holds voxel 64 w + i of the row
template <typename T>
__global__ __launch_bounds__(MORPH_THREADS) void morph_pack_kernel(const T *labels, const int *table, int n_table, MorphGeom g,
                                                                   unsigned long long outside_word, unsigned long long *plane) {
    const int lane = threadIdx.x & 63, waves = (int)gridDim.x * (MORPH_THREADS / 64);
    for (long long i = (long long)blockIdx.x * (MORPH_THREADS / 64) + (threadIdx.x >> 6); i < g.n_words; i += waves) {
        const int w = (int)(i % g.W), row = (int)(i / g.W), z = 64 * w + lane;
        const bool in = z < g.b.bz && fh_in_set(labels, morph_voxel(g, row, z), table, n_table);
        const unsigned long long word = __ballot(in);
        if (lane == 0) plane[i] = morph_fix_tail(word, w, g.b.bz, outside_word);
    }
}

// c. one step.  Thread t holds word t of the plane, w fastest, so the lanes of a wave hold adjacent words of a row: the
// carry bits of words w - 1 and w + 1 come from the neighbouring lanes; only a wave's first and last lane load them (when
// the row goes on there), and a row's first and last word take `outside`.  Every lane runs every shuffle: threads past the
// plane's end skip the loads and the store only.
template <int RANK, int OP>
__global__ __launch_bounds__(MORPH_THREADS) void morph_step_kernel(const unsigned long long *__restrict__ src,
                                                                   unsigned long long *__restrict__ dst, MorphGeom g, int axes,
                                                                   int outside) {
    const long long t = (long long)blockIdx.x * MORPH_THREADS + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const bool live = t < g.n_words;
    const int w = live ? (int)(t % g.W) : 0, row = live ? (int)(t / g.W) : 0, y = row % g.b.by, x = row / g.b.by;
    const uint64_t out_word = outside ? ~0ull : 0ull, zmask = (axes & 4) ? ~0ull : 0ull;
    uint64_t c[9];
    uint32_t ph[9], nl[9];
#pragma unroll
    for (int r = 0; r < 9; ++r) {
        c[r] = 0; ph[r] = nl[r] = 0;
        if (!morph_row_used<RANK>(r)) continue;
        const int dx = morph_row_dx(r), dy = morph_row_dy(r), xx = x + dx, yy = y + dy;
        const bool neutral = (dx && !(axes & 1)) || (dy && !(axes & 2));
        const bool inside = live && !neutral && xx >= 0 && xx < g.b.bx && yy >= 0 && yy < g.b.by;
        const unsigned long long *rp = src + (long long)(xx * g.b.by + yy) * g.W;
        const uint64_t fallback = neutral ? morph_neutral<OP>() : out_word;
        c[r] = inside ? rp[w] : fallback;
        if (!morph_row_spread<RANK>(r)) continue;
        const uint32_t up = (uint32_t)__shfl_up((int)(c[r] >> 63), 1), down = (uint32_t)__shfl_down((int)(c[r] & 1), 1);
        const uint32_t edge = (uint32_t)(fallback & 1);             // what lies past the row's ends, or the whole row's value
        if (!inside) { ph[r] = nl[r] = edge; continue; }
        ph[r] = w == 0 ? (uint32_t)outside : lane == 0 ? (uint32_t)(rp[w - 1] >> 63) : up;
        nl[r] = w == g.W - 1 ? (uint32_t)outside : lane == 63 ? (uint32_t)(rp[w + 1] & 1) : down;
    }
    if (live) dst[t] = morph_fix_tail(morph_word<RANK, OP>(c, ph, nl, zmask), w, g.b.bz, out_word);
}

// d. the label rule.  ADD (dilation, closing): voxels of the result outside the set whose value is background become fill.
// Otherwise (erosion, opening): voxels of the set outside the result become background.
template <typename T, bool ADD>
__global__ __launch_bounds__(MORPH_THREADS) void morph_apply_kernel(T *labels, const int *table, int n_table, MorphGeom g,
                                                                    const unsigned long long *__restrict__ plane, T background, T fill,
                                                                    unsigned long long *changed) {
    const int lane = threadIdx.x & 63, waves = (int)gridDim.x * (MORPH_THREADS / 64);
    int cnt = 0;
    for (long long i = (long long)blockIdx.x * (MORPH_THREADS / 64) + (threadIdx.x >> 6); i < g.n_words; i += waves) {
        const int w = (int)(i % g.W), row = (int)(i / g.W), z = 64 * w + lane;
        const uint64_t valid = morph_valid_bits(w, g.b.bz), word = plane[i];
        if (ADD ? (word & valid) == 0 : (word & valid) == valid) continue;       // wave-uniform: nothing to add / to remove here
        if (z >= g.b.bz) continue;
        const bool bit = (word >> lane) & 1;
        const int vox = morph_voxel(g, row, z);
        const T v = labels[vox];
        const bool in = (int)v < n_table && table[v] >= 0;
        if (ADD ? (bit && !in && v == background) : (in && !bit)) {
            labels[vox] = ADD ? fill : background;
            ++cnt;
        }
    }
    cnt = wave_sum(cnt);
    if (lane == 0 && cnt) atomicAdd(changed, (unsigned long long)cnt);
}

template <int RANK, int OP>
void launch_step(HipCall &call, const unsigned long long *src, unsigned long long *dst, const MorphGeom &g, int axes, int outside) {
    const unsigned blocks = (unsigned)(((long long)g.n_words + MORPH_THREADS - 1) / MORPH_THREADS);
    call.launch(morph_step_kernel<RANK, OP>, dim3(blocks), dim3(MORPH_THREADS), 0, src, dst, g, axes, outside);
}

void launch_step(HipCall &call, int rank, int step, const unsigned long long *src, unsigned long long *dst, const MorphGeom &g, int axes,
                 int outside) {
    if (step == MORPH_DILATE) {
        if (rank == 1) launch_step<1, MORPH_DILATE>(call, src, dst, g, axes, outside);
        else if (rank == 2) launch_step<2, MORPH_DILATE>(call, src, dst, g, axes, outside);
        else launch_step<3, MORPH_DILATE>(call, src, dst, g, axes, outside);
    } else {
        if (rank == 1) launch_step<1, MORPH_ERODE>(call, src, dst, g, axes, outside);
        else if (rank == 2) launch_step<2, MORPH_ERODE>(call, src, dst, g, axes, outside);
        else launch_step<3, MORPH_ERODE>(call, src, dst, g, axes, outside);
    }
}

}  // namespace

extern "C" {

int fnn_binary_morphology(void *labels, int label_dtype, const int64_t shape[3], const int32_t *group_of_label, int n_table,
                          int op, int connectivity, int iterations, int border_value, int background_label, int fill_label,
                          int axes, int64_t *changed, void *stream) {
    const char *who = "fnn_binary_morphology";
    if (!shape) return fnn_fail(FNN_E_INVALID, "NULL shape");
    if (int rc = fnn_check_label_dtype(label_dtype)) return rc;
    if (op < FNN_MORPH_DILATE || op > FNN_MORPH_CLOSE) return fnn_fail(FNN_E_INVALID, "op must be FNN_MORPH_DILATE, ERODE, OPEN or CLOSE (0..3)");
    const int rank = morph_rank(connectivity);
    if (!rank) return fnn_fail(FNN_E_INVALID, "connectivity must be 6, 18 or 26");
    if (iterations < 1 || iterations > MORPH_MAX_ITERATIONS) return fnn_fail(FNN_E_INVALID, "iterations must be 1..1024");
    if (border_value != 0 && border_value != 1) return fnn_fail(FNN_E_INVALID, "border_value must be 0 or 1");
    const int max_label = label_dtype == FNN_LABEL_U16 ? 65535 : 255;
    const bool adds = morph_adds(op);
    if (background_label < 0 || background_label > max_label) return fnn_fail(FNN_E_INVALID, "background_label outside the label dtype");
    if (adds && (fill_label < 0 || fill_label > max_label)) return fnn_fail(FNN_E_INVALID, "fill_label outside the label dtype");
    if (adds && fill_label == background_label) return fnn_fail(FNN_E_INVALID, "fill_label equals background_label");
    if (axes < 1 || axes > 7) return fnn_fail(FNN_E_INVALID, "axes must be 1..7 (bit a: the structure spans axis a)");
    if (shape[0] < 0 || shape[1] < 0 || shape[2] < 0) return fnn_fail(FNN_E_INVALID, "negative shape");
    if (n_table < 0 || (n_table > 0 && !group_of_label)) return fnn_fail(FNN_E_INVALID, "bad label-set table");
    for (int v = 0; v < n_table; ++v)
        if (group_of_label[v] < -1 || group_of_label[v] > 0) return fnn_fail(FNN_E_INVALID, "group_of_label entry outside [-1, 0]");
    if (changed) *changed = 0;
    if (shape[0] == 0 || shape[1] == 0 || shape[2] == 0) return FNN_OK;
    if (shape[0] > INT_MAX || shape[1] > INT_MAX || shape[2] > INT_MAX || shape[0] * shape[1] > INT_MAX ||
        shape[0] * shape[1] * shape[2] > INT_MAX)
        return fnn_failf(FNN_E_UNSUPPORTED, "%s: more than 2^31 - 1 voxels", who);
    if (int rc = fnn_need_dev(who, {labels}, "a device label map")) return rc;
    const int n_tab = n_table < max_label + 1 ? n_table : max_label + 1;
    if (n_tab == 0 && border_value == 0) return FNN_OK;                          // S is empty and nothing grows from the border
    const FHVolume vol{(int)shape[0], (int)shape[1], (int)shape[2]};

    // the small block: raw box [6] | pad [2] | voxels of S | changed | table [n_tab]
    DevBuf small;
    if (!small.alloc(48 + (size_t)n_tab * 4)) return fnn_fail(FNN_E_HIP, "hipMalloc failed (fnn_binary_morphology: the label table)");
    int *raw = small.as<int>(), *table = small.as<int>(48);
    unsigned long long *count = small.as<unsigned long long>(32), *nchanged = small.as<unsigned long long>(40);
    HipCall call(stream);
    call.fill(raw, 0xff, 32);
    call.fill(count, 0, 16);
    if (n_tab) call.copy(table, group_of_label, (size_t)n_tab * 4, hipMemcpyHostToDevice);

    FHBox b{0, 0, 0, vol.X, vol.Y, vol.Z};
    if (border_value == 0) {
        fnn_by_label(label_dtype, [&](auto lt) {
            using LT = decltype(lt);
            fh_launch_box(call, (const LT *)labels, table, n_tab, vol, raw, count);
        });
        struct { int raw[8]; unsigned long long count; } found;
        call.copy(&found, raw, 40, hipMemcpyDeviceToHost);
        if (!call.sync()) return call.fail();
        if (!fh_box_from_raw(found.raw, shape, b)) return FNN_OK;                 // S is empty
        if (adds) b = morph_grow_box(b, shape, iterations, axes);
    }
    const int64_t words = morph_plane_words(b);                                  // <= voxels of the box: fits an int
    const MorphGeom g{b, vol.Y, vol.Z, morph_row_words(b.bz), (int)words};

    DevBuf planes;
    if (!planes.alloc((size_t)words * 16)) return fnn_fail(FNN_E_HIP, "hipMalloc failed (fnn_binary_morphology: 2 bits per voxel of the box)");
    unsigned long long *cur = planes.as<unsigned long long>(), *next = planes.as<unsigned long long>((size_t)words * 8);
    const unsigned long long outside_word = border_value ? ~0ull : 0ull;
    const unsigned wave_blocks = (unsigned)((words + MORPH_THREADS / 64 - 1) / (MORPH_THREADS / 64));
    const dim3 grid(wave_blocks < MORPH_MAX_BLOCKS ? wave_blocks : MORPH_MAX_BLOCKS), block(MORPH_THREADS);
    fnn_by_label(label_dtype, [&](auto lt) {
        using LT = decltype(lt);
        call.launch(morph_pack_kernel<LT>, grid, block, 0, (const LT *)labels, (const int *)table, n_tab, g, outside_word, cur);
    });
    int step[2];
    const int runs = morph_phases(op, step);
    for (int k = 0; k < runs; ++k)
        for (int it = 0; it < iterations; ++it) {
            launch_step(call, rank, step[k], cur, next, g, axes, border_value);
            unsigned long long *t = cur; cur = next; next = t;
        }
    fnn_by_label(label_dtype, [&](auto lt) {
        using LT = decltype(lt);
        if (adds)
            call.launch(morph_apply_kernel<LT, true>, grid, block, 0, (LT *)labels, (const int *)table, n_tab, g,
                        (const unsigned long long *)cur, (LT)background_label, (LT)fill_label, nchanged);
        else
            call.launch(morph_apply_kernel<LT, false>, grid, block, 0, (LT *)labels, (const int *)table, n_tab, g,
                        (const unsigned long long *)cur, (LT)background_label, (LT)0, nchanged);
    });
    unsigned long long hchanged = 0;
    if (changed) call.copy(&hchanged, nchanged, 8, hipMemcpyDeviceToHost);
    if (!call.sync()) return call.fail();
    if (changed) *changed = (int64_t)hchanged;
    return FNN_OK;
}

}  // extern "C"
