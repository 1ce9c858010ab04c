// fill_holes_host.cpp - the box arithmetic of fnn_fill_holes (csrc/fill_holes_box.h, host code without HIP) as a plain
// executable.  tests/test_fill_holes_host_cpu.py builds it with the host compiler under the address and undefined-behaviour
// sanitizers and runs it; nothing is loaded into Python.  For small random volumes and every border_axes it does on the host what
// the entry does on the device - the raw box of the set as the box kernel leaves it, the complement's face-connected components
// inside the box only, a component open iff it has a voxel on a face that fh_open_faces names - and compares the holes with a
// flood fill of the whole volume from the faces of the border axes: the claim that labelling inside the box is exact.  Every
// array is a heap block of its exact size.  Exit code 0 and one line per check; the first failed check ends the program with 1.
#include "../fast-nnunet_amd/csrc/fill_holes_box.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

static int n_checks = 0;
#define CHECK(cond)                                                                           \
    do {                                                                                      \
        if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); exit(1); }   \
        ++n_checks;                                                                           \
    } while (0)

static unsigned long long rng_state = 33;
static unsigned rnd() {
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (unsigned)(rng_state >> 33);
}

// face-connected flood fill of `free` voxels of a [X][Y][Z] block from the seeds (reached = 1)
static void flood(const std::vector<char> &free_, int X, int Y, int Z, std::vector<int> &stack, std::vector<char> &reached) {
    while (!stack.empty()) {
        const int i = stack.back();
        stack.pop_back();
        const int z = i % Z, y = (i / Z) % Y, x = i / (Z * Y);
        const int nb[6][3] = {{x - 1, y, z}, {x + 1, y, z}, {x, y - 1, z}, {x, y + 1, z}, {x, y, z - 1}, {x, y, z + 1}};
        for (const auto &q : nb) {
            if (q[0] < 0 || q[1] < 0 || q[2] < 0 || q[0] >= X || q[1] >= Y || q[2] >= Z) continue;
            const int j = (q[0] * Y + q[1]) * Z + q[2];
            if (free_[j] && !reached[j]) { reached[j] = 1; stack.push_back(j); }
        }
    }
}

static void one_volume(const int64_t shape[3], const std::vector<char> &in_set, int border_axes) {
    const int X = (int)shape[0], Y = (int)shape[1], Z = (int)shape[2], n = X * Y * Z;
    // the truth: complement voxels not reached from the volume's faces along the border axes
    std::vector<char> free_(n), reached(n, 0);
    std::vector<int> stack;
    for (int i = 0; i < n; ++i) free_[i] = !in_set[i];
    for (int i = 0; i < n; ++i) {
        const int c[3] = {i / (Z * Y), (i / Z) % Y, i % Z};
        bool border = false;
        for (int a = 0; a < 3; ++a) border |= ((border_axes >> a) & 1) && (c[a] == 0 || c[a] == shape[a] - 1);
        if (border && free_[i]) { reached[i] = 1; stack.push_back(i); }
    }
    flood(free_, X, Y, Z, stack, reached);
    // the entry's way: the raw box as the box kernel leaves it ...
    int raw[6] = {-1, -1, -1, -1, -1, -1};
    long long count = 0;
    for (int i = 0; i < n; ++i) {
        if (!in_set[i]) continue;
        const int c[3] = {i / (Z * Y), (i / Z) % Y, i % Z};
        for (int a = 0; a < 3; ++a) {
            if ((int)shape[a] - 1 - c[a] > raw[a]) raw[a] = (int)shape[a] - 1 - c[a];
            if (c[a] > raw[3 + a]) raw[3 + a] = c[a];
        }
        ++count;
    }
    FHBox b;
    if (!fh_box_from_raw(raw, shape, b)) {                       // an empty set has no hole
        CHECK(count == 0);
        return;
    }
    CHECK(b.x0 >= 0 && b.y0 >= 0 && b.z0 >= 0 && b.bx >= 1 && b.by >= 1 && b.bz >= 1);
    CHECK(b.x0 + b.bx <= X && b.y0 + b.by <= Y && b.z0 + b.bz <= Z && fh_box_voxels(b) >= count);
    // ... every voxel of the set inside it, every complement voxel outside it reached in the truth
    for (int i = 0; i < n; ++i) {
        const int x = i / (Z * Y), y = (i / Z) % Y, z = i % Z;
        const bool inside = x >= b.x0 && x < b.x0 + b.bx && y >= b.y0 && y < b.y0 + b.by && z >= b.z0 && z < b.z0 + b.bz;
        if (in_set[i]) CHECK(inside);
        else if (!inside) CHECK(reached[i]);
    }
    // ... the complement inside the box, flooded from the faces fh_open_faces opens
    const int open = fh_open_faces(b, shape, border_axes);
    const int nb = (int)fh_box_voxels(b);
    std::vector<char> bfree(nb), breached(nb, 0);
    for (int l = 0; l < nb; ++l) {
        const int z = l % b.bz, y = (l / b.bz) % b.by, x = l / (b.bz * b.by);
        bfree[l] = free_[((b.x0 + x) * Y + (b.y0 + y)) * Z + (b.z0 + z)];
        const int on = (x == 0 ? 1 : 0) | (x == b.bx - 1 ? 2 : 0) | (y == 0 ? 4 : 0) | (y == b.by - 1 ? 8 : 0) | (z == 0 ? 16 : 0) |
                       (z == b.bz - 1 ? 32 : 0);
        if ((on & open) && bfree[l]) { breached[l] = 1; stack.push_back(l); }
    }
    flood(bfree, b.bx, b.by, b.bz, stack, breached);
    for (int l = 0; l < nb; ++l) {
        const int z = l % b.bz, y = (l / b.bz) % b.by, x = l / (b.bz * b.by);
        CHECK(breached[l] == reached[((b.x0 + x) * Y + (b.y0 + y)) * Z + (b.z0 + z)]);
    }
}

int main() {
    {                                                              // the faces, written out
        const int64_t shape[3] = {10, 10, 10};
        const FHBox inner{2, 3, 4, 3, 3, 3}, low{0, 0, 0, 3, 3, 3}, whole{0, 0, 0, 10, 10, 10}, plane{0, 2, 2, 1, 5, 5};
        const int64_t flat[3] = {1, 10, 10};
        CHECK(fh_open_faces(inner, shape, 7) == 63 && fh_open_faces(inner, shape, 1) == 63);
        CHECK(fh_open_faces(low, shape, 7) == 63 && fh_open_faces(low, shape, 6) == (2 | 4 | 8 | 16 | 32));
        CHECK(fh_open_faces(whole, shape, 7) == 63 && fh_open_faces(whole, shape, 2) == (4 | 8) && fh_open_faces(whole, shape, 4) == (16 | 32));
        CHECK(fh_open_faces(plane, flat, 6) == (4 | 8 | 16 | 32) && fh_open_faces(plane, flat, 7) == 63);
        const int raw[6] = {7, 6, 5, 4, 5, 6};
        FHBox b;
        CHECK(fh_box_from_raw(raw, shape, b) && b.x0 == 2 && b.y0 == 3 && b.z0 == 4 && b.bx == 3 && b.by == 3 && b.bz == 3 && fh_box_voxels(b) == 27);
        const int none[6] = {-1, -1, -1, -1, -1, -1};
        CHECK(!fh_box_from_raw(none, shape, b));
        const FHBox big{0, 0, 0, 2048, 1024, 1023};
        CHECK(fh_box_voxels(big) == 2048ll * 1024 * 1023);
        printf("ok faces: open faces and the raw box on written-out cases\n");
    }
    int volumes = 0;
    for (int trial = 0; trial < 400; ++trial) {
        const int64_t shape[3] = {1 + rnd() % 6, 1 + rnd() % 6, 1 + rnd() % 7};
        const int n = (int)(shape[0] * shape[1] * shape[2]);
        const unsigned density = 20 + rnd() % 75;                 // per cent of the voxels in the set
        std::vector<char> in_set(n);
        for (int i = 0; i < n; ++i) in_set[i] = rnd() % 100 < density;
        // half of the trials: the set confined to a sub-block, so that the box lies inside the volume
        if (trial & 1)
            for (int i = 0; i < n; ++i) {
                const int c[3] = {i / (int)(shape[2] * shape[1]), (i / (int)shape[2]) % (int)shape[1], i % (int)shape[2]};
                for (int a = 0; a < 3; ++a)
                    if (shape[a] > 2 && (c[a] == 0 || c[a] == shape[a] - 1)) in_set[i] = 0;
            }
        for (int axes = 1; axes <= 7; ++axes) one_volume(shape, in_set, axes);
        ++volumes;
    }
    printf("ok boxes: %d random volumes x 7 border masks - the holes found inside the box are the holes of the volume\n", volumes);
    printf("%d checks passed\n", n_checks);
    return 0;
}
