// morph_core_host.cpp - the rule of fnn_binary_morphology (csrc/morph_core.h, code that compiles without HIP) as a plain
// executable.  tests/test_morph_core_host_cpu.py builds it with the host compiler under the address and undefined-behaviour
// sanitizers and runs it; nothing is loaded into Python.  For small random volumes it does on the host what the entry does on
// the device - the set's box (grown for the adding operations, the whole volume with border_value 1), the mask packed into
// 64-bit words, morph_word on every word of the plane for every one-step pass of the operation - and compares every bit with a
// byte-wise brute force over the whole volume whose outside reads as border_value: inside the box the bits must be equal, and
// outside the box the brute force must have left nothing (the claim that the box is enough).  After the pack and after every
// pass every word is checked to be in the one form morph_core.h asks for (the bits past a row's end hold `outside`).  Every
// array is a heap block of its exact size.  Exit code 0 and one line per check; the first failed check ends the program with 1.
#include "../fast-nnunet_amd/csrc/morph_core.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

static long long n_checks = 0;
#define CHECK(cond)                                                                           \
    do {                                                                                      \
        if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); exit(1); }   \
        ++n_checks;                                                                           \
    } while (0)

static unsigned long long rng_state = 34;
static unsigned rnd() {
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (unsigned)(rng_state >> 33);
}

typedef std::vector<unsigned char> Bytes;

// one byte-wise step over the whole volume: step MORPH_DILATE / MORPH_ERODE, the structure of `rank` over `axes`
static Bytes brute_step(const Bytes &m, const int64_t shape[3], int step, int rank, int axes, int border) {
    const int X = (int)shape[0], Y = (int)shape[1], Z = (int)shape[2];
    Bytes out(m.size());
    for (int x = 0; x < X; ++x)
        for (int y = 0; y < Y; ++y)
            for (int z = 0; z < Z; ++z) {
                bool any = false, all = true;
                for (int dx = -1; dx <= 1; ++dx)
                    for (int dy = -1; dy <= 1; ++dy)
                        for (int dz = -1; dz <= 1; ++dz) {
                            if ((dx && !(axes & 1)) || (dy && !(axes & 2)) || (dz && !(axes & 4))) continue;
                            if (abs(dx) + abs(dy) + abs(dz) > rank) continue;
                            const int a = x + dx, b = y + dy, c = z + dz;
                            const bool in = a >= 0 && a < X && b >= 0 && b < Y && c >= 0 && c < Z;
                            const bool v = in ? m[((size_t)a * Y + b) * Z + c] != 0 : border != 0;
                            any |= v; all &= v;
                        }
                out[((size_t)x * Y + y) * Z + z] = step == MORPH_DILATE ? any : all;
            }
    return out;
}

static void step_plane(int rank, int step, const uint64_t *src, uint64_t *dst, const FHBox &b, int axes, int outside) {
    if (step == MORPH_DILATE) {
        if (rank == 1) morph_step_plane<1, MORPH_DILATE>(src, dst, b, axes, outside);
        else if (rank == 2) morph_step_plane<2, MORPH_DILATE>(src, dst, b, axes, outside);
        else morph_step_plane<3, MORPH_DILATE>(src, dst, b, axes, outside);
    } else {
        if (rank == 1) morph_step_plane<1, MORPH_ERODE>(src, dst, b, axes, outside);
        else if (rank == 2) morph_step_plane<2, MORPH_ERODE>(src, dst, b, axes, outside);
        else morph_step_plane<3, MORPH_ERODE>(src, dst, b, axes, outside);
    }
}

static void check_form(const std::vector<uint64_t> &plane, const FHBox &b, int outside) {
    const int W = morph_row_words(b.bz);
    const uint64_t valid = morph_valid_bits(W - 1, b.bz), want = outside ? ~valid : 0ull;
    bool ok = true;
    for (int64_t row = 0; row < (int64_t)b.bx * b.by; ++row) ok &= (plane[(size_t)(row * W + W - 1)] & ~valid) == want;
    CHECK(ok);
}

// the whole operation both ways; returns false when the set is empty and the entry would end after the box pass
static bool one_case(const int64_t shape[3], const Bytes &in_set, int op, int conn, int n, int border, int axes) {
    const int X = (int)shape[0], Y = (int)shape[1], Z = (int)shape[2], rank = morph_rank(conn);
    CHECK(rank >= 1 && rank <= 3);
    int step[2];
    const int runs = morph_phases(op, step);
    Bytes truth = in_set;
    for (int k = 0; k < runs; ++k)
        for (int it = 0; it < n; ++it) truth = brute_step(truth, shape, step[k], rank, axes, border);

    FHBox b{0, 0, 0, X, Y, Z};
    if (border == 0) {
        int raw[6] = {-1, -1, -1, -1, -1, -1};
        for (int x = 0; x < X; ++x)
            for (int y = 0; y < Y; ++y)
                for (int z = 0; z < Z; ++z) {
                    if (!in_set[((size_t)x * Y + y) * Z + z]) continue;
                    const int c[3] = {x, y, z};
                    for (int a = 0; a < 3; ++a) {
                        if ((int)shape[a] - 1 - c[a] > raw[a]) raw[a] = (int)shape[a] - 1 - c[a];
                        if (c[a] > raw[3 + a]) raw[3 + a] = c[a];
                    }
                }
        if (!fh_box_from_raw(raw, shape, b)) {
            bool none = true;
            for (unsigned char v : truth) none &= !v;
            CHECK(none);                                                  // an empty set stays empty
            return false;
        }
        if (morph_adds(op)) b = morph_grow_box(b, shape, n, axes);
        CHECK(b.x0 >= 0 && b.y0 >= 0 && b.z0 >= 0 && b.x0 + b.bx <= X && b.y0 + b.by <= Y && b.z0 + b.bz <= Z);
    }
    const int W = morph_row_words(b.bz);
    const uint64_t out_word = border ? ~0ull : 0ull;
    std::vector<uint64_t> cur((size_t)morph_plane_words(b)), next(cur.size());
    for (int x = 0; x < b.bx; ++x)
        for (int y = 0; y < b.by; ++y)
            for (int w = 0; w < W; ++w) {
                uint64_t word = 0;
                for (int i = 0; i < 64 && 64 * w + i < b.bz; ++i)
                    if (in_set[((size_t)(b.x0 + x) * Y + b.y0 + y) * Z + b.z0 + 64 * w + i]) word |= 1ull << i;
                cur[((size_t)x * b.by + y) * W + w] = morph_fix_tail(word, w, b.bz, out_word);
            }
    check_form(cur, b, border);
    for (int k = 0; k < runs; ++k)
        for (int it = 0; it < n; ++it) {
            step_plane(rank, step[k], cur.data(), next.data(), b, axes, border);
            cur.swap(next);
            check_form(cur, b, border);
        }
    bool same = true, nothing_outside = true;
    for (int x = 0; x < X; ++x)
        for (int y = 0; y < Y; ++y)
            for (int z = 0; z < Z; ++z) {
                const bool t = truth[((size_t)x * Y + y) * Z + z] != 0;
                const int lx = x - b.x0, ly = y - b.y0, lz = z - b.z0;
                if (lx < 0 || lx >= b.bx || ly < 0 || ly >= b.by || lz < 0 || lz >= b.bz) { nothing_outside &= !t; continue; }
                same &= t == (((cur[((size_t)lx * b.by + ly) * W + (lz >> 6)] >> (lz & 63)) & 1) != 0);
            }
    CHECK(same);
    CHECK(nothing_outside);
    return true;
}

static Bytes random_set(const int64_t shape[3], unsigned percent) {
    Bytes m((size_t)(shape[0] * shape[1] * shape[2]));
    for (auto &v : m) v = rnd() % 100 < percent;
    return m;
}

static const int CONN[3] = {6, 18, 26};

int main() {
    // ---- the word rule: every op, rank, border value and n = 1..3 on rows of one word, two words, with and without a tail
    {
        const int rows[7] = {1, 63, 64, 65, 127, 128, 130};
        const int64_t xy[4][2] = {{3, 4}, {1, 5}, {4, 1}, {1, 1}};                 // extents of 1 along x, along y, along both
        long long cases = 0, tails = 0;
        for (int zi = 0; zi < 7; ++zi)
            for (int s = 0; s < 4; ++s) {
                const int64_t shape[3] = {xy[s][0], xy[s][1], rows[zi]};
                const unsigned dens[3] = {15, 50, 88};
                const Bytes m = random_set(shape, dens[(zi + s) % 3]);
                for (int op = 0; op < 4; ++op)
                    for (int c = 0; c < 3; ++c)
                        for (int border = 0; border < 2; ++border)
                            for (int n = 1; n <= 3; ++n) {
                                const int axes = shape[0] == 1 && (n & 1) ? 6 : 7;  // a 2-D map, and (1, Y, Z) as a 3-D one
                                if (one_case(shape, m, op, CONN[c], n, border, axes)) { ++cases; tails += rows[zi] % 64 != 0; }
                            }
            }
        CHECK(cases > 1500 && tails > 1000);
        printf("ok words: %lld cases of op x rank x border x n on rows of 1, 63, 64, 65, 127, 128 and 130 voxels equal the byte-wise brute force\n", cases);
        printf("ok tails: %lld of them with bits past the row's end; every plane holds `outside` there after the pack and after every pass\n", tails);
    }
    // ---- the helpers of the one form
    {
        CHECK(morph_row_words(1) == 1 && morph_row_words(64) == 1 && morph_row_words(65) == 2 && morph_row_words(130) == 3);
        CHECK(morph_valid_bits(0, 64) == ~0ull && morph_valid_bits(0, 1) == 1ull && morph_valid_bits(1, 65) == 1ull && morph_valid_bits(2, 130) == 3ull);
        CHECK(morph_valid_bits(1, 64) == 0ull && morph_valid_bits(0, 130) == ~0ull);
        CHECK(morph_fix_tail(~0ull, 2, 130, 0ull) == 3ull && morph_fix_tail(0ull, 2, 130, ~0ull) == ~3ull && morph_fix_tail(5ull, 0, 64, ~0ull) == 5ull);
        // a stale tail bit is what goes wrong: erosion fed a 0 past the end removes the row's last voxel, dilation fed a 1 grows one
        uint64_t c[9] = {0}; uint32_t ph[9] = {0}, nl[9] = {0};
        for (int r = 0; r < 9; ++r) { c[r] = ~0ull; ph[r] = nl[r] = 1; }
        CHECK((morph_word<1, MORPH_ERODE>(c, ph, nl, ~0ull)) == ~0ull);
        c[4] = ~0ull >> 1;                                                          // bit 63 of the centre word is 0
        CHECK((morph_word<1, MORPH_ERODE>(c, ph, nl, ~0ull)) == (~0ull >> 2));      // bits 62 and 63 go
        CHECK((morph_word<1, MORPH_ERODE>(c, ph, nl, 0ull)) == (~0ull >> 1));       // without the z axis only bit 63
        for (int r = 0; r < 9; ++r) { c[r] = 0; ph[r] = nl[r] = 0; }
        nl[4] = 1;                                                                  // the next word starts with a voxel
        CHECK((morph_word<1, MORPH_DILATE>(c, ph, nl, ~0ull)) == 1ull << 63);
        nl[4] = 0; nl[0] = 1;                                                       // the same in a diagonal row: rank 3 only
        CHECK((morph_word<2, MORPH_DILATE>(c, ph, nl, ~0ull)) == 0ull && (morph_word<3, MORPH_DILATE>(c, ph, nl, ~0ull)) == 1ull << 63);
        c[0] = 2;
        CHECK((morph_word<1, MORPH_DILATE>(c, ph, nl, ~0ull)) == 0ull && (morph_word<2, MORPH_DILATE>(c, ph, nl, ~0ull)) == 2ull);
        const int64_t shape[3] = {10, 10, 100};
        const FHBox b{2, 0, 90, 3, 4, 5}, g = morph_grow_box(b, shape, 3, 7), g2 = morph_grow_box(b, shape, 3, 6);
        CHECK(g.x0 == 0 && g.bx == 8 && g.y0 == 0 && g.by == 7 && g.z0 == 87 && g.bz == 11);
        CHECK(g2.x0 == 2 && g2.bx == 3 && g2.by == 7 && g2.bz == 11);
        int step[2];
        CHECK(morph_phases(0, step) == 1 && step[0] == MORPH_DILATE && morph_phases(1, step) == 1 && step[0] == MORPH_ERODE);
        CHECK(morph_phases(2, step) == 2 && step[0] == MORPH_ERODE && step[1] == MORPH_DILATE);
        CHECK(morph_phases(3, step) == 2 && step[0] == MORPH_DILATE && step[1] == MORPH_ERODE);
        CHECK(morph_adds(0) && !morph_adds(1) && !morph_adds(2) && morph_adds(3) && morph_rank(7) == 0 && morph_rank(18) == 2);
    }
    // ---- boxes that touch no face, the low face, the high face or both faces of the volume, per axis
    {
        const int64_t shape[3] = {6, 6, 70};
        const int lo[4][3] = {{2, 2, 3}, {0, 0, 0}, {3, 3, 60}, {0, 0, 0}}, hi[4][3] = {{4, 4, 67}, {3, 3, 9}, {6, 6, 70}, {6, 6, 70}};
        long long cases = 0;
        for (int fx = 0; fx < 4; ++fx)
            for (int fy = 0; fy < 4; ++fy)
                for (int fz = 0; fz < 4; ++fz) {
                    Bytes m((size_t)(shape[0] * shape[1] * shape[2]), 0);
                    // the corners of the range are set, so the box is the range; the rest at random
                    for (int x = lo[fx][0]; x < hi[fx][0]; ++x)
                        for (int y = lo[fy][1]; y < hi[fy][1]; ++y)
                            for (int z = lo[fz][2]; z < hi[fz][2]; ++z) {
                                const bool corner = (x == lo[fx][0] || x == hi[fx][0] - 1) && (y == lo[fy][1] || y == hi[fy][1] - 1) &&
                                                    (z == lo[fz][2] || z == hi[fz][2] - 1);
                                m[((size_t)x * shape[1] + y) * shape[2] + z] = corner || rnd() % 100 < 60;
                            }
                    for (int op = 0; op < 4; ++op)
                        for (int c = 0; c < 3; ++c)
                            for (int border = 0; border < 2; ++border)
                                cases += one_case(shape, m, op, CONN[c], 2, border, 7);
                }
        CHECK(cases == 64 * 4 * 3 * 2);
        const Bytes none((size_t)(shape[0] * shape[1] * shape[2]), 0);
        CHECK(!one_case(shape, none, 0, 26, 2, 0, 7) && !one_case(shape, none, 3, 6, 1, 0, 7));
        CHECK(one_case(shape, none, 0, 26, 2, 1, 7) && one_case(shape, none, 2, 6, 3, 1, 7));     // border 1 grows from the faces
        printf("ok boxes: %lld cases on boxes touching 0, 1 or 2 faces of the volume per axis; nothing of the result lies outside the box\n", cases);
    }
    printf("%lld checks passed\n", n_checks);
    return 0;
}
