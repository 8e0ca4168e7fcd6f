// The bit grid of csrc/occupancy.hip and csrc/region.hip: one bit per cell of an axis-aligned box.  THE statement of the
// convention for the device and the C ABI (the Python side: mvip_nerf_amd/bitgrid.py; restated for the tests in
// tests/occupancy_numpy.py and tests/region_numpy.py).
//
// The box [bmin, bmax] is cut into (cx, cy, cz) cells, each 1..512.  Cell of a point p, per axis in fp32:
// f = floorf((p - bmin) * inv), inv = cells / (bmax - bmin) rounded once on the host; p is in the box iff 0 <= f < c on all
// three axes (a NaN or infinite coordinate fails the comparison: outside).  Linear cell l = (ix * cy + iy) * cz + iz
// (z fastest), bit l & 31 of 32-bit word l >> 5, (cx cy cz + 31) / 32 words, unused tail bits zero.
// What a clear bit or a point outside the box MEANS is the user's: occupancy's keep(p), region's inside(p).
#pragma once
#include "common.h"

namespace mvip {
namespace bitgrid {

struct Grid {                                // the words travel beside it
    float bx, by, bz, ix, iy, iz;
    int cx, cy, cz;
};

// linear cell of a point, -1 outside the box
__device__ __forceinline__ int cell_of(const Grid &g, float x, float y, float z) {
    const float fx = floorf((x - g.bx) * g.ix), fy = floorf((y - g.by) * g.iy), fz = floorf((z - g.bz) * g.iz);
    const bool in_box = fx >= 0.f && fx < (float)g.cx && fy >= 0.f && fy < (float)g.cy && fz >= 0.f && fz < (float)g.cz;
    return in_box ? ((int)fx * g.cy + (int)fy) * g.cz + (int)fz : -1;
}

__device__ __forceinline__ bool cell_bit(const unsigned *__restrict__ words, int l) { return (words[l >> 5] >> (l & 31)) & 1u; }

// (i, j, k) of linear index l in an [*, ny, nz] array, z fastest (cells here, lattice points in csrc/mcubes.hip)
__device__ __forceinline__ void linear_ijk(int l, int ny, int nz, int &i, int &j, int &k) {
    const int sx = ny * nz;
    i = l / sx;
    const int r = l - i * sx;
    j = r / nz;
    k = r - j * nz;
}

// ---- host side: what every entry point checks of its grid arguments ---------------------------------------------------
static inline bool cells_ok(int cx, int cy, int cz) {
    return cx >= 1 && cx <= 512 && cy >= 1 && cy <= 512 && cz >= 1 && cz <= 512;
}
static inline int n_words(int cx, int cy, int cz) { return (int)(((int64_t)cx * cy * cz + 31) / 32); }
// box = (bmin[3], inv[3]), cells[3] in host memory, words on the device
static inline bool grid_from_args(const float *box, const int *cells, const int *words, Grid &g) {
    if (!box || !cells || !words || !cells_ok(cells[0], cells[1], cells[2])) return false;
    for (int a = 0; a < 6; ++a)
        if (!finite(box[a])) return false;
    if (!(box[3] > 0.f) || !(box[4] > 0.f) || !(box[5] > 0.f)) return false;
    g = Grid{box[0], box[1], box[2], box[3], box[4], box[5], cells[0], cells[1], cells[2]};
    return true;
}

}  // namespace bitgrid
}  // namespace mvip
