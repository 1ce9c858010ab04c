// morph_core.h - the rule of fnn_binary_morphology (morph.hip) that the kernels and the host test share: the geometry of the
// packed bit planes, the box they cover, the order of the one-step passes of an operation, and one step of dilation or erosion
// on one 64-bit word.  Compiles as plain C++ (tests/morph_core_host.cpp) and as HIP device code.
//
// The definition is scipy.ndimage's binary_dilation / binary_erosion / binary_opening / binary_closing with
// structure = generate_binary_structure(ndim, rank), iterations = n and border_value = b: n iterations equal n one-step passes
// over a map whose outside reads as b (opening: n erosions then n dilations, closing: n dilations then n erosions).
//
// Planes.  The mask lives in a box [bx][by][bz] of the volume as rows of W = ceil(bz / 64) words; bit i of word w of row
// (x, y) is voxel z = 64 w + i of the box.  Every plane is kept in ONE form, in every phase: the bits of the last word past
// the end of the row hold `outside`, the value everything outside the box reads as.  Pack and every step end with
// morph_fix_tail, so a step's z-neighbour read across the end of a row needs no case of its own, erosion cannot be fed a
// stale 0 and dilation cannot grow a phantom out of a stale 1.
//
// Outside.  With border_value 0 everything outside the box reads 0: beyond a volume face that is the border value, and
// inside the volume the box (the set's bounding box, grown by n for the adding operations) holds every voxel the mask can reach
// in any phase - dilate^k(M) stays inside M's box grown by k, and with a zero border erosion and opening only shrink.  With
// border_value 1 the box is the whole volume and every face of it is a volume face that reads 1.  So `outside` is one bit per
// call, equal to border_value, and no face of the box needs to know where it lies.
//
// Axes.  The structure spans the axes of `axes` (bit 0 x, 1 y, 2 z).  A neighbour across an axis outside `axes` is not part
// of the structure: its row reads as the operation's neutral word (0 for dilation, ~0 for erosion) and a z-neighbour is
// masked by zmask = 0.  An offset (dx, dy, dz) over the spanned axes belongs to the structure iff |dx| + |dy| + |dz| <= rank,
// which on two axes gives the cross for rank 1 and the full 3 x 3 for rank 2 and 3, as generate_binary_structure(2, rank).
#pragma once
#include "fill_holes_box.h"
#include <cstdint>

#if defined(__HIPCC__)
#define MORPH_HD __host__ __device__ __forceinline__
#else
#define MORPH_HD inline
#endif

enum { MORPH_DILATE = 0, MORPH_ERODE = 1 };                 // one step; the operations of the ABI are runs of these

constexpr int MORPH_MAX_ITERATIONS = 1024;

// ---- the operation as at most two runs of one-step passes: step[k] repeated n times, k < the returned count
inline int morph_phases(int op, int step[2]) {               // op: FNN_MORPH_DILATE 0, ERODE 1, OPEN 2, CLOSE 3
    switch (op) {
    case 0: step[0] = MORPH_DILATE; return 1;
    case 1: step[0] = MORPH_ERODE; return 1;
    case 2: step[0] = MORPH_ERODE; step[1] = MORPH_DILATE; return 2;
    default: step[0] = MORPH_DILATE; step[1] = MORPH_ERODE; return 2;
    }
}
inline bool morph_adds(int op) { return op == 0 || op == 3; }       // dilation and closing only add, the other two only remove
inline int morph_rank(int connectivity) { return connectivity == 6 ? 1 : connectivity == 18 ? 2 : connectivity == 26 ? 3 : 0; }

// ---- the box: the set's box grown by `grow` voxels along each axis of `axes`, clipped to the volume
inline FHBox morph_grow_box(const FHBox &b, const int64_t shape[3], int grow, int axes) {
    int lo[3] = {b.x0, b.y0, b.z0}, ext[3] = {b.bx, b.by, b.bz};
    for (int a = 0; a < 3; ++a) {
        if (!((axes >> a) & 1)) continue;
        const int64_t l = (int64_t)lo[a] - grow, h = (int64_t)lo[a] + ext[a] + grow;
        const int nl = (int)(l < 0 ? 0 : l), nh = (int)(h > shape[a] ? shape[a] : h);
        lo[a] = nl; ext[a] = nh - nl;
    }
    return FHBox{lo[0], lo[1], lo[2], ext[0], ext[1], ext[2]};
}

// ---- the planes
MORPH_HD int morph_row_words(int bz) { return (bz + 63) >> 6; }
MORPH_HD int64_t morph_plane_words(const FHBox &b) { return (int64_t)b.bx * b.by * morph_row_words(b.bz); }
// the bits of word w of a row of bz voxels that are voxels
MORPH_HD uint64_t morph_valid_bits(int w, int bz) {
    const int left = bz - 64 * w;
    return left >= 64 ? ~0ull : left <= 0 ? 0ull : (1ull << left) - 1;
}
// the one form of a plane word: bits past the end of the row hold `outside`
MORPH_HD uint64_t morph_fix_tail(uint64_t word, int w, int bz, uint64_t outside_word) {
    const uint64_t valid = morph_valid_bits(w, bz);
    return (word & valid) | (outside_word & ~valid);
}
template <int OP> MORPH_HD uint64_t morph_neutral() { return OP == MORPH_DILATE ? 0ull : ~0ull; }

// ---- the structure, row by row: row r = (dx + 1) * 3 + (dy + 1) of the 3 x 3 rows around the output word's
constexpr int morph_row_dx(int r) { return r / 3 - 1; }
constexpr int morph_row_dy(int r) { return r % 3 - 1; }
constexpr int morph_row_dist(int r) { return (r / 3 == 1 ? 0 : 1) + (r % 3 == 1 ? 0 : 1); }
template <int RANK> constexpr bool morph_row_used(int r) { return morph_row_dist(r) <= RANK; }            // any offset of it
template <int RANK> constexpr bool morph_row_spread(int r) { return morph_row_dist(r) + 1 <= RANK; }      // its dz = +-1 too

// a word with its two z-neighbours: prev_hi is bit 63 of the word before it in the row, next_lo bit 0 of the word after
template <int OP> MORPH_HD uint64_t morph_zspread(uint64_t c, uint32_t prev_hi, uint32_t next_lo, uint64_t zmask) {
    const uint64_t below = (c << 1) | (uint64_t)(prev_hi & 1u), above = (c >> 1) | ((uint64_t)(next_lo & 1u) << 63);
    return OP == MORPH_DILATE ? c | (zmask & (below | above)) : c & (~zmask | (below & above));
}

// One step on one word.  c[r]: word w of row r; prev_hi[r] / next_lo[r]: the carry bits of words w - 1 and w + 1 of that row
// (read only for the rows that morph_row_spread names); rows the structure does not use are not read at all.  Whatever lies
// outside the box arrives as `outside`, a row across an axis outside `axes` as morph_neutral<OP>() - the caller's loader says
// which, this function has no case for either.
template <int RANK, int OP>
MORPH_HD uint64_t morph_word(const uint64_t c[9], const uint32_t prev_hi[9], const uint32_t next_lo[9], uint64_t zmask) {
    uint64_t acc = morph_zspread<OP>(c[4], prev_hi[4], next_lo[4], zmask);
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int r = 0; r < 9; ++r) {
        if (r == 4 || !morph_row_used<RANK>(r)) continue;
        const uint64_t v = morph_row_spread<RANK>(r) ? morph_zspread<OP>(c[r], prev_hi[r], next_lo[r], zmask) : c[r];
        acc = OP == MORPH_DILATE ? acc | v : acc & v;
    }
    return acc;
}

// One step of a whole plane, the loop the step kernel runs with one thread per word: the host test's device under test, and
// the statement of what the kernel's loader must deliver.  src and dst: morph_plane_words(b) words, src in the one form.
template <int RANK, int OP>
inline void morph_step_plane(const uint64_t *src, uint64_t *dst, const FHBox &b, int axes, int outside) {
    const int W = morph_row_words(b.bz);
    const uint64_t out_word = outside ? ~0ull : 0ull, zmask = (axes & 4) ? ~0ull : 0ull;
    for (int x = 0; x < b.bx; ++x)
        for (int y = 0; y < b.by; ++y)
            for (int w = 0; w < W; ++w) {
                uint64_t c[9];
                uint32_t ph[9], nl[9];
                for (int r = 0; r < 9; ++r) {
                    const int dx = morph_row_dx(r), dy = morph_row_dy(r), xx = x + dx, yy = y + dy;
                    c[r] = 0; ph[r] = nl[r] = 0;
                    if (!morph_row_used<RANK>(r)) continue;
                    if ((dx && !(axes & 1)) || (dy && !(axes & 2))) {
                        c[r] = morph_neutral<OP>(); ph[r] = nl[r] = (uint32_t)(c[r] & 1);
                    } else if (xx < 0 || xx >= b.bx || yy < 0 || yy >= b.by) {
                        c[r] = out_word; ph[r] = nl[r] = (uint32_t)outside;
                    } else {
                        const uint64_t *row = src + ((int64_t)xx * b.by + yy) * W;
                        c[r] = row[w];
                        ph[r] = w > 0 ? (uint32_t)(row[w - 1] >> 63) : (uint32_t)outside;
                        nl[r] = w + 1 < W ? (uint32_t)(row[w + 1] & 1) : (uint32_t)outside;
                    }
                }
                dst[((int64_t)x * b.by + y) * W + w] = morph_fix_tail(morph_word<RANK, OP>(c, ph, nl, zmask), w, b.bz, out_word);
            }
}
