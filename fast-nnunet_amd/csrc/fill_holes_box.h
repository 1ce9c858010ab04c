// fill_holes_box.h - the box arithmetic of fnn_fill_holes (postprocess.hip), host code without HIP: what the box pass's
// result means, which faces of the box open a complement component to the volume's border, and whether anything is left to
// do.  tests/fill_holes_host.cpp compiles this header alone.
//
// The complement of the set S is labelled only inside S's bounding box.  A complement component that lies inside the box is
// a hole unless it reaches the volume's border along an axis of border_axes.  It can do so in two ways, and both go through
// a face of the box:
//   * the box face lies on the volume's face along an axis a of border_axes: the component touches that border itself;
//   * the box face lies strictly inside the volume: the voxel beyond it is outside the box, hence in the complement, and the
//     slab of the volume beyond that face holds no voxel of S and spans the volume's full extent along the other two axes
//     and up to the volume's face along its own - it touches a face of the volume along every axis, one of border_axes among
//     them (border_axes is not 0).
// A box face that lies on a volume face along an axis outside border_axes is no border and leads nowhere.  So a face opens
// iff its axis is in border_axes or it lies strictly inside the volume; with all three axes in border_axes (a 3-D map) this
// is "every box face", and for a depth-1 volume with the first axis cleared (a 2-D map) the two faces of that axis stay shut.
#pragma once
#include <cstdint>

struct FHBox {
    int x0, y0, z0;                    // first voxel of the box in the volume [X][Y][Z]
    int bx, by, bz;                    // its extents
};

// what the box pass leaves: raw[k] = dim_k - 1 - lowest coordinate (k = 0..2), raw[3 + k] = highest coordinate, every entry
// -1 when no voxel belongs to S
inline bool fh_box_from_raw(const int raw[6], const int64_t shape[3], FHBox &b) {
    if (raw[3] < 0) return false;
    b.x0 = (int)shape[0] - 1 - raw[0]; b.y0 = (int)shape[1] - 1 - raw[1]; b.z0 = (int)shape[2] - 1 - raw[2];
    b.bx = raw[3] - b.x0 + 1; b.by = raw[4] - b.y0 + 1; b.bz = raw[5] - b.z0 + 1;
    return true;
}

inline int64_t fh_box_voxels(const FHBox &b) { return (int64_t)b.bx * b.by * b.bz; }

// bit 2 a: the low face of axis a opens a component, bit 2 a + 1: the high face (border_axes: bit a - axis a has borders)
inline int fh_open_faces(const FHBox &b, const int64_t shape[3], int border_axes) {
    const int lo[3] = {b.x0, b.y0, b.z0}, ext[3] = {b.bx, b.by, b.bz};
    int open = 0;
    for (int a = 0; a < 3; ++a) {
        const bool border = (border_axes >> a) & 1;
        if (border || lo[a] > 0) open |= 1 << (2 * a);
        if (border || (int64_t)lo[a] + ext[a] < shape[a]) open |= 2 << (2 * a);
    }
    return open;
}
