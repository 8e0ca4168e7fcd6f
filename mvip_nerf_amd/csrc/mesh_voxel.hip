// Voxelisation of an indexed triangle mesh into the bit grid of csrc/bitgrid_device.h (beyond the reference: MVIP-NeRF has no
// mesh export, so nothing here has a reference call site; ops.mesh_voxelize_surface / mesh_voxelize_solid, mesh.voxelize,
// Region.from_mesh, OccupancyGrid.from_mesh).  The way back from a cleaned mesh to the renderer: the cells its faces touch
// (SURFACE) and the cells inside it (SOLID).  THE statement of both definitions; restated for the tests in
// tests/voxel_numpy.py.  Everything is fp64 on widened fp32 inputs plus integers, every expression associates as written (the
// library is built with -ffp-contract=off; fp64 + - * / floor and rint are correctly rounded), so the restatement agrees BIT
// FOR BIT.
//
// LATTICE COORDINATES.  A grid is (bmin, inv, cells) as BitGrid.box() hands it over: fp32 bmin and inv, cells 1..512 per axis.
// A vertex p has g = (double(p) - double(bmin)) * double(inv) per axis.  Cell i spans [i, i + 1), its centre is i + 0.5.
// Output: l = (ix cy + iy) cz + iz, bit l & 31 of word l >> 5, tail bits zero.  A face index outside [0, Nv) raises the flag
// and drops the face (it is not counted in `dropped`).
//
// SOLID, the parity fill of Schwarz and Seidel 2010 ("Fast parallel surface and solid voxelization on GPUs").  `axes` names the
// walked column axes: one of x, y, z, or all three ('majority').  For column axis a the raster axes are (b, c) = (y, z), (z, x),
// (x, y) for a = x, y, z.
//   A face is DROPPED WHOLE (from every walked axis, counted once in `dropped`) unless all nine g are finite and |256 g| <= 2^22
//   on every raster axis of every walked axis (for 'majority': on all three axes), compared in fp64 before the conversion.  The
//   bound is the guard band of csrc/raster.hip: it keeps every edge function below 2^47, exact in int64 and in fp64.
//   Per walked axis a:
//   1. Snap.  X_k = rint(256 g_kb), Y_k = rint(256 g_kc), ties to even: 8 sub-cell bits, integers from here on.
//   2. Orient.  A2 = (X1 - X0)(Y2 - Y0) - (Y1 - Y0)(X2 - X0).  A2 = 0: the face is skipped for this axis (not counted).
//      A2 < 0: vertices 1 and 2 are swapped (X, Y and g_a), so that A2 > 0 from here on.
//   3. Cover.  The sample of column (x, y), 0 <= x < cells_b, 0 <= y < cells_c, is (sx, sy) = (256 x + 128, 256 y + 128).  For
//      the edge from vertex i to j opposite k (k = 0: 1 -> 2, k = 1: 2 -> 0, k = 2: 0 -> 1), with (ex, ey) = (Xj - Xi, Yj - Yi):
//      E_k = ex (sy - Yi) - ey (sx - Xi); the sample is covered iff for every k E_k > 0, or E_k = 0 and (ey < 0, or ey = 0 and
//      ex > 0) -- the top-left ownership rule of csrc/raster.hip.  It does not depend on which face the edge belongs to, so two
//      faces that share an edge never both cover a sample and never both miss it.
//   4. Depth.  depth = ((E0 g0_a + E1 g1_a) + E2 g2_a) / A2 in fp64; k = floor(depth - 0.5) + 1, the first cell whose centre
//      lies strictly beyond the crossing.  k >= cells_a: no mark.  k < 0: k = 0 (a crossing in front of the box flips the
//      whole column).  One bit is XORed at cell (x, y, k) of the crossing grid of axis a.
//   After all faces cell i of a column is inside for axis a iff the XOR of the crossing bits 0..i of its column is 1;
//   odd_columns[a] = the number of columns whose total parity is odd (0 for an axis not walked).  A single axis gives its own
//   result; 'majority' sets a cell iff at least two of the three per-axis results have it set.  All marks are integer XOR: the
//   result does not depend on the order of the atomics.
//   What this guarantees.  Snapping moves each vertex by at most 2^-9 of a cell on each raster axis, so the snapped triangle's
//   point of equal barycentrics lies within 2^-9 sqrt 2 of the true one, across the column direction and not along it (g_a is
//   not snapped).  Seen from a cell centre, a column's crossing sequence through the snapped mesh is the sequence of the true
//   mesh along a line displaced by less than 2^-9 sqrt 2 < 2^-8 of a cell; a centre farther than 2^-8 of a cell from the
//   surface of a closed mesh is on the same side of the displaced surface, and, since the ownership rule counts every crossing
//   of a closed snapped mesh exactly once (columns are even: odd_columns = 0 inside the guard band), its parity is the exact
//   inside / outside answer, on every axis and so from the majority.  Removing one face changes, on axis a, only the columns
//   whose sample the snapped face covers, all of them inside the face's bounding box dilated by 2^-9 on b and c; a cell is
//   changed on axis a only if its centre is inside that dilated box on (b, c).  Where the three axes agreed before, the
//   majority changes only where two axes change: the centre is then inside the dilated box on all three axes.  (Where they
//   disagreed -- only within 2^-8 of a cell of the surface -- one axis can tip the vote.)  A single axis leaks whole column
//   segments.
//
// SURFACE, the exact triangle-box overlap of Akenine-Moller 2001 with a margin m = 2^-12 of a cell.
//   A face with a non-finite g is dropped and counted in `dropped`.
//   Candidate cells per axis: floor(min g - m) .. floor(max g + m), clipped to 0 .. cells - 1.
//   Face constants from g: e0 = g1 - g0, e1 = g2 - g1, e2 = g0 - g2; n = e0 x e1 = (e0y e1z - e0z e1y, e0z e1x - e0x e1z,
//   e0x e1y - e0y e1x).  For a candidate with centre c = (ix + .5, iy + .5, iz + .5): v_k = g_k - c, h = 0.5 + m.  The cell is
//   set iff none of these separates:
//     the normal:  |(n_x v0x + n_y v0y) + n_z v0z| > h ((|n_x| + |n_y|) + |n_z|);
//     for each edge e = e_j, with p_k over the three vertices and separated iff min p > r or max p < -r:
//       unit_x x e:  p_k = e_y v_kz - e_z v_ky,  r = h (|e_y| + |e_z|);
//       unit_y x e:  p_k = e_z v_kx - e_x v_kz,  r = h (|e_z| + |e_x|);
//       unit_z x e:  p_k = e_x v_ky - e_y v_kx,  r = h (|e_x| + |e_y|).
//   The three box axes are the candidate range itself.  A degenerate face is its segment or point under the same tests (n = 0
//   never separates).  Marks are integer OR.
//   What this guarantees: every fp32 point q on a face that cell_of (csrc/bitgrid_device.h) places in the box is placed in a
//   set cell.  cell_of forms floorf(fl(fl(q - bmin) inv)) in fp32: two roundings of relative size 2^-24 on a value below 512,
//   so its argument is within 2^-14 of a cell of q's exact lattice coordinate and the cell it names holds a point within 2^-14
//   of the face on that axis.  The box of half-width 0.5 + 2^-12 around that cell's centre therefore meets the face with 2^-12 -
//   2^-14 to spare, which also covers the fp64 rounding of the tests: with |g| <= 2^22 each p and r carries an error below
//   2^-28 |e|, against a margin of 2^-12 |e|.  (A face with |g| beyond 2^38 has no such bound.)
//
// SHAPE.  voxel_surface_kernel: one thread per face, 256 per workgroup; a candidate range of at most 64 cells is walked by its
// own thread, larger ones by the whole wave afterwards (the lanes that hold one are balloted, the nine g and the range are
// broadcast in turn, the 64 lanes stride over the range's cells).  voxel_crossings_kernel: one thread per (face, walked axis);
// a raster box of at most 16 samples by its own thread, larger ones by the wave as 8 x 8 tiles, the scheme of csrc/raster.hip.
// No thread loops alone over more than those counts.  The integer edge set-up is restated here and not taken from
// csrc/raster_device.h: that one is __device__ only and samples at 256 x, this one is __host__ __device__ (a stand-alone host
// program walks the same functions) and samples at 256 x + 128.  The crossing grids are laid out [ix, iy, (cz + 31) / 32]
// words, z fastest and padded to words, for every axis: the prefix parity along x and along y is then a running XOR of whole
// words down a strided column (one thread per word column, 32 cells at a time, coalesced across threads), and along z a prefix
// XOR inside each word by five shifts with a carry across at most 16 words.  voxel_combine_kernel: one thread per output word
// gathers its up to 32 row segments from the padded rows, takes the majority and writes the word -- no two threads write one
// word.  No LDS, no scratch memory, no float atomics; every loop's trip count is bounded by the grid (<= 512 slabs, <= 16
// words, <= 32 segments, a candidate range inside the grid); every index is clamped into the grid before use, offsets fit int
// (512^3 = 2^27).
#include "bitgrid_device.h"
#include <math.h>

#define MVIP_HD __host__ __device__ __forceinline__

namespace mvip {
namespace voxel {

constexpr int BLOCK = 256;
constexpr int SMALL_CELLS = 64;              // the largest candidate range, in cells, that a thread walks alone
constexpr int SMALL_SAMPLES = 16;            // the largest raster box, in samples, that a thread walks alone
constexpr double BAND = 4194304.0;           // 2^22 sub-cell units
constexpr double MARGIN = 1.0 / 4096.0;      // 2^-12 of a cell
constexpr int64_t INT_MAX64 = 2147483647;
constexpr int AXES_MAJORITY = 3;
constexpr int N_COUNTERS = 5;                // flag, dropped, odd columns x / y / z

struct Lattice {
    double bx, by, bz, ix, iy, iz;
    int cx, cy, cz;
};

struct Face {                                // the nine lattice coordinates
    double x0, y0, z0, x1, y1, z1, x2, y2, z2;
};

MVIP_HD bool finite64(double x) { return fabs(x) <= 1.7976931348623157e308; }
MVIP_HD double sel(int k, double x, double y, double z) { return k == 0 ? x : (k == 1 ? y : z); }
MVIP_HD int sel(int k, int x, int y, int z) { return k == 0 ? x : (k == 1 ? y : z); }
MVIP_HD int words_per_row(int cz) { return (cz + 31) >> 5; }

MVIP_HD void lattice_face(const Lattice &L, const float *__restrict__ verts, int i0, int i1, int i2, Face &f) {
    const float *p0 = verts + 3 * (long long)i0, *p1 = verts + 3 * (long long)i1, *p2 = verts + 3 * (long long)i2;
    f.x0 = ((double)p0[0] - L.bx) * L.ix; f.y0 = ((double)p0[1] - L.by) * L.iy; f.z0 = ((double)p0[2] - L.bz) * L.iz;
    f.x1 = ((double)p1[0] - L.bx) * L.ix; f.y1 = ((double)p1[1] - L.by) * L.iy; f.z1 = ((double)p1[2] - L.bz) * L.iz;
    f.x2 = ((double)p2[0] - L.bx) * L.ix; f.y2 = ((double)p2[1] - L.by) * L.iy; f.z2 = ((double)p2[2] - L.bz) * L.iz;
}

MVIP_HD bool face_finite(const Face &f) {
    return finite64(f.x0) && finite64(f.y0) && finite64(f.z0) && finite64(f.x1) && finite64(f.y1) && finite64(f.z1) &&
           finite64(f.x2) && finite64(f.y2) && finite64(f.z2);
}

// ---- SOLID ------------------------------------------------------------------------------------------------------------------
MVIP_HD bool in_band(double u0, double u1, double u2) {
    return fabs(256.0 * u0) <= BAND && fabs(256.0 * u1) <= BAND && fabs(256.0 * u2) <= BAND;      // a NaN fails
}

// DROPPED WHOLE of the header, negated
MVIP_HD bool face_kept(const Face &f, int axes) {
    if (!face_finite(f)) return false;
    const bool bx = in_band(f.x0, f.x1, f.x2), by = in_band(f.y0, f.y1, f.y2), bz = in_band(f.z0, f.z1, f.z2);
    return (axes == 0 || bx) && (axes == 1 || by) && (axes == 2 || bz);
}

// a kept face set up for column axis a: A2 > 0
struct Tri {
    int X0, Y0, X1, Y1, X2, Y2;
    double d0, d1, d2;                       // g_a of the three vertices
    long long A2;
};

// false: A2 = 0, the face is skipped for this axis
MVIP_HD bool setup(const Face &f, int a, Tri &t) {
    const int b = a == 2 ? 0 : a + 1, c = b == 2 ? 0 : b + 1;
    t.X0 = (int)rint(256.0 * sel(b, f.x0, f.y0, f.z0)); t.Y0 = (int)rint(256.0 * sel(c, f.x0, f.y0, f.z0));
    t.X1 = (int)rint(256.0 * sel(b, f.x1, f.y1, f.z1)); t.Y1 = (int)rint(256.0 * sel(c, f.x1, f.y1, f.z1));
    t.X2 = (int)rint(256.0 * sel(b, f.x2, f.y2, f.z2)); t.Y2 = (int)rint(256.0 * sel(c, f.x2, f.y2, f.z2));
    t.d0 = sel(a, f.x0, f.y0, f.z0);
    t.d1 = sel(a, f.x1, f.y1, f.z1);
    t.d2 = sel(a, f.x2, f.y2, f.z2);
    t.A2 = (long long)(t.X1 - t.X0) * (t.Y2 - t.Y0) - (long long)(t.Y1 - t.Y0) * (t.X2 - t.X0);
    if (t.A2 == 0) return false;
    if (t.A2 < 0) {
        const int x = t.X1, y = t.Y1;
        const double d = t.d1;
        t.X1 = t.X2; t.Y1 = t.Y2; t.d1 = t.d2;
        t.X2 = x; t.Y2 = y; t.d2 = d;
        t.A2 = -t.A2;
    }
    return true;
}

// the columns (x0 .. x0 + w - 1, y0 .. y0 + h - 1) whose sample lies in the snapped bounding box, clipped to the grid; false: none
MVIP_HD bool sample_box(const Tri &t, int cb, int cc, int &x0, int &y0, int &w, int &h) {
    const int xmin = min(t.X0, min(t.X1, t.X2)), xmax = max(t.X0, max(t.X1, t.X2));
    const int ymin = min(t.Y0, min(t.Y1, t.Y2)), ymax = max(t.Y0, max(t.Y1, t.Y2));
    x0 = max(0, (xmin + 127) >> 8);          // 256 x + 128 >= xmin; integers within +-2^22
    y0 = max(0, (ymin + 127) >> 8);
    w = min(cb - 1, (xmax - 128) >> 8) - x0 + 1;
    h = min(cc - 1, (ymax - 128) >> 8) - y0 + 1;
    return w > 0 && h > 0;
}

// the three edge functions at the sample of column (x, y), their steps per column, and nb_k = 0 where edge k owns its zero
struct Edges {
    long long E0, E1, E2, dx0, dx1, dx2, dy0, dy1, dy2;
    int nb0, nb1, nb2;
};

MVIP_HD void edge(int Xi, int Yi, int Xj, int Yj, long long sx, long long sy, long long &E, long long &dx, long long &dy, int &nb) {
    const long long ex = Xj - Xi, ey = Yj - Yi;
    E = ex * (sy - Yi) - ey * (sx - Xi);
    dx = -256 * ey;
    dy = 256 * ex;
    nb = (ey < 0 || (ey == 0 && ex > 0)) ? 0 : 1;
}

MVIP_HD void edges_at(const Tri &t, int x, int y, Edges &e) {
    const long long sx = 256ll * x + 128, sy = 256ll * y + 128;
    edge(t.X1, t.Y1, t.X2, t.Y2, sx, sy, e.E0, e.dx0, e.dy0, e.nb0);
    edge(t.X2, t.Y2, t.X0, t.Y0, sx, sy, e.E1, e.dx1, e.dy1, e.nb1);
    edge(t.X0, t.Y0, t.X1, t.Y1, sx, sy, e.E2, e.dx2, e.dy2, e.nb2);
}

// Cover and Depth of the header for one sample: the cell k of the mark, -1 for none
MVIP_HD int crossing_cell(long long E0, long long E1, long long E2, int nb0, int nb1, int nb2, double d0, double d1, double d2,
                          double A2, int ca) {
    if (((E0 - nb0) | (E1 - nb1) | (E2 - nb2)) < 0) return -1;
    const double depth = (((double)E0 * d0 + (double)E1 * d1) + (double)E2 * d2) / A2;
    const double k = floor(depth - 0.5) + 1.0;
    if (!(k < (double)ca)) return -1;
    return k < 0.0 ? 0 : (int)k;
}

// word and bit of cell (x, y, k) of the (b, c, a) frame in the padded crossing grid [cx, cy, wz]
MVIP_HD void crossing_bit(int a, int x, int y, int k, int cy, int wz, int &word, unsigned &bit) {
    // a = 0: (ix, iy, iz) = (k, x, y); a = 1: (y, k, x); a = 2: (x, y, k)
    const int ix = sel(a, k, y, x), iy = sel(a, x, k, y), iz = sel(a, y, x, k);
    word = (ix * cy + iy) * wz + (iz >> 5);
    bit = 1u << (iz & 31);
}

// ---- SURFACE ----------------------------------------------------------------------------------------------------------------
// the clipped candidate range of one axis: false where it is empty
MVIP_HD bool candidate_range(double g0, double g1, double g2, int c, int &lo, int &n) {
    const double a = floor(fmin(g0, fmin(g1, g2)) - MARGIN), b = floor(fmax(g0, fmax(g1, g2)) + MARGIN);
    const double l = fmax(a, 0.0), h = fmin(b, (double)(c - 1));
    if (!(l <= h)) return false;
    lo = (int)l;
    n = (int)h - lo + 1;
    return true;
}

MVIP_HD bool axis_separates(double p0, double p1, double p2, double r) {
    return fmin(p0, fmin(p1, p2)) > r || fmax(p0, fmax(p1, p2)) < -r;
}

// the nine cross-product axes of one edge e against the three vertices v_k
MVIP_HD bool edge_separates(double ex, double ey, double ez, double v0x, double v0y, double v0z, double v1x, double v1y, double v1z,
                            double v2x, double v2y, double v2z, double h) {
    if (axis_separates(ey * v0z - ez * v0y, ey * v1z - ez * v1y, ey * v2z - ez * v2y, h * (fabs(ey) + fabs(ez)))) return true;
    if (axis_separates(ez * v0x - ex * v0z, ez * v1x - ex * v1z, ez * v2x - ex * v2z, h * (fabs(ez) + fabs(ex)))) return true;
    return axis_separates(ex * v0y - ey * v0x, ex * v1y - ey * v1x, ex * v2y - ey * v2x, h * (fabs(ex) + fabs(ey)));
}

// the overlap test of the header for the cell (ix, iy, iz), a candidate
MVIP_HD bool overlaps(const Face &f, int ix, int iy, int iz) {
    const double h = 0.5 + MARGIN;
    const double cx = (double)ix + 0.5, cy = (double)iy + 0.5, cz = (double)iz + 0.5;
    const double e0x = f.x1 - f.x0, e0y = f.y1 - f.y0, e0z = f.z1 - f.z0;
    const double e1x = f.x2 - f.x1, e1y = f.y2 - f.y1, e1z = f.z2 - f.z1;
    const double e2x = f.x0 - f.x2, e2y = f.y0 - f.y2, e2z = f.z0 - f.z2;
    const double nx = e0y * e1z - e0z * e1y, ny = e0z * e1x - e0x * e1z, nz = e0x * e1y - e0y * e1x;
    const double v0x = f.x0 - cx, v0y = f.y0 - cy, v0z = f.z0 - cz;
    const double v1x = f.x1 - cx, v1y = f.y1 - cy, v1z = f.z1 - cz;
    const double v2x = f.x2 - cx, v2y = f.y2 - cy, v2z = f.z2 - cz;
    if (fabs((nx * v0x + ny * v0y) + nz * v0z) > h * ((fabs(nx) + fabs(ny)) + fabs(nz))) return false;
    if (edge_separates(e0x, e0y, e0z, v0x, v0y, v0z, v1x, v1y, v1z, v2x, v2y, v2z, h)) return false;
    if (edge_separates(e1x, e1y, e1z, v0x, v0y, v0z, v1x, v1y, v1z, v2x, v2y, v2z, h)) return false;
    return !edge_separates(e2x, e2y, e2z, v0x, v0y, v0z, v1x, v1y, v1z, v2x, v2y, v2z, h);
}

#ifdef __HIPCC__
// ---- kernels ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BLOCK) void voxel_clear_kernel(unsigned *__restrict__ words, const int n, int *__restrict__ counters) {
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i < n) words[i] = 0u;
    if (i < N_COUNTERS && counters != nullptr) counters[i] = 0;
}

__global__ __launch_bounds__(BLOCK) void voxel_surface_kernel(const float *__restrict__ verts, const int *__restrict__ faces,
                                                             const int Nv, const int F, const Lattice L, unsigned *words,
                                                             int *counters) {
    const int fi = blockIdx.x * BLOCK + threadIdx.x;
    Face f{};
    int x0 = 0, y0 = 0, z0 = 0, nx = 0, ny = 0, nz = 0;
    bool valid = false;
    if (fi < F) {
        const int i0 = faces[3ll * fi], i1 = faces[3ll * fi + 1], i2 = faces[3ll * fi + 2];
        if ((unsigned)i0 >= (unsigned)Nv || (unsigned)i1 >= (unsigned)Nv || (unsigned)i2 >= (unsigned)Nv) {
            atomicOr(counters, 1);
        } else {
            lattice_face(L, verts, i0, i1, i2, f);
            if (!face_finite(f)) {
                atomicAdd(counters + 1, 1);
            } else {
                valid = candidate_range(f.x0, f.x1, f.x2, L.cx, x0, nx);
                valid = candidate_range(f.y0, f.y1, f.y2, L.cy, y0, ny) && valid;
                valid = candidate_range(f.z0, f.z1, f.z2, L.cz, z0, nz) && valid;
            }
        }
    }
    const int n = valid ? nx * ny * nz : 0;                 // <= 512^3 = 2^27
    const bool large = n > SMALL_CELLS;

    if (valid && !large) {                                  // at most SMALL_CELLS cells, by this thread alone
        for (int i = 0; i < n; ++i) {
            const int kz = i % nz, t = i / nz;
            const int ix = x0 + t / ny, iy = y0 + t % ny, iz = z0 + kz;
            if (overlaps(f, ix, iy, iz)) {
                const int l = (ix * L.cy + iy) * L.cz + iz;
                atomicOr(words + (l >> 5), 1u << (l & 31));
            }
        }
    }

    // the large ranges, one after the other, by the whole wave: every lane of the wave arrives here
    unsigned long long pending = __ballot(large);
    const int lane = threadIdx.x & 63;
    while (pending) {
        const int src = __ffsll((long long)pending) - 1;
        pending &= pending - 1;
        Face s;
        s.x0 = __shfl(f.x0, src, 64); s.y0 = __shfl(f.y0, src, 64); s.z0 = __shfl(f.z0, src, 64);
        s.x1 = __shfl(f.x1, src, 64); s.y1 = __shfl(f.y1, src, 64); s.z1 = __shfl(f.z1, src, 64);
        s.x2 = __shfl(f.x2, src, 64); s.y2 = __shfl(f.y2, src, 64); s.z2 = __shfl(f.z2, src, 64);
        const int sx0 = __shfl(x0, src, 64), sy0 = __shfl(y0, src, 64), sz0 = __shfl(z0, src, 64);
        const int sny = __shfl(ny, src, 64), snz = __shfl(nz, src, 64), sn = __shfl(n, src, 64);
        for (int i = lane; i < sn; i += 64) {
            const int kz = i % snz, t = i / snz;
            const int ix = sx0 + t / sny, iy = sy0 + t % sny, iz = sz0 + kz;
            if (overlaps(s, ix, iy, iz)) {
                const int l = (ix * L.cy + iy) * L.cz + iz;
                atomicOr(words + (l >> 5), 1u << (l & 31));
            }
        }
    }
}

// one sample of the crossings kernel: the mark, if any
__device__ __forceinline__ void cross(long long E0, long long E1, long long E2, int nb0, int nb1, int nb2, double d0, double d1,
                                      double d2, double A2, int a, int ca, int x, int y, int cy, int wz, unsigned *grid) {
    const int k = crossing_cell(E0, E1, E2, nb0, nb1, nb2, d0, d1, d2, A2, ca);
    if (k < 0) return;
    int word;
    unsigned bit;
    crossing_bit(a, x, y, k, cy, wz, word, bit);
    atomicXor(grid + word, bit);
}

// axes: 0..2 one axis, its grid at scratch; 3: the three grids one after the other
__global__ __launch_bounds__(BLOCK) void voxel_crossings_kernel(const float *__restrict__ verts, const int *__restrict__ faces,
                                                               const int Nv, const int F, const Lattice L, const int axes,
                                                               const int blocks_per_axis, const int grid_words, unsigned *scratch,
                                                               int *counters) {
    const int slot = blockIdx.x / blocks_per_axis;          // uniform in the workgroup
    const int a = axes == AXES_MAJORITY ? slot : axes;
    const int fi = (blockIdx.x - slot * blocks_per_axis) * BLOCK + threadIdx.x;
    const int b = a == 2 ? 0 : a + 1, c = b == 2 ? 0 : b + 1;
    const int ca = sel(a, L.cx, L.cy, L.cz), cb = sel(b, L.cx, L.cy, L.cz), cc = sel(c, L.cx, L.cy, L.cz);
    const int wz = words_per_row(L.cz);
    unsigned *const grid = scratch + (long long)slot * grid_words;

    Tri t{};
    int bx0 = 0, by0 = 0, bw = 0, bh = 0;
    bool valid = false;
    if (fi < F) {
        const int i0 = faces[3ll * fi], i1 = faces[3ll * fi + 1], i2 = faces[3ll * fi + 2];
        if ((unsigned)i0 >= (unsigned)Nv || (unsigned)i1 >= (unsigned)Nv || (unsigned)i2 >= (unsigned)Nv) {
            if (slot == 0) atomicOr(counters, 1);
        } else {
            Face f;
            lattice_face(L, verts, i0, i1, i2, f);
            if (!face_kept(f, axes)) {
                if (slot == 0) atomicAdd(counters + 1, 1);
            } else if (setup(f, a, t)) {
                valid = sample_box(t, cb, cc, bx0, by0, bw, bh);
            }
        }
    }
    const bool large = valid && bw * bh > SMALL_SAMPLES;    // <= 512 x 512

    if (valid && !large) {                                  // at most SMALL_SAMPLES samples, by this thread alone
        Edges e;
        edges_at(t, bx0, by0, e);
        const double A2 = (double)t.A2;
        for (int y = 0; y < bh; ++y) {
            long long E0 = e.E0, E1 = e.E1, E2 = e.E2;
            for (int x = 0; x < bw; ++x) {
                cross(E0, E1, E2, e.nb0, e.nb1, e.nb2, t.d0, t.d1, t.d2, A2, a, ca, bx0 + x, by0 + y, L.cy, wz, grid);
                E0 += e.dx0; E1 += e.dx1; E2 += e.dx2;
            }
            e.E0 += e.dy0; e.E1 += e.dy1; e.E2 += e.dy2;
        }
    }

    // the large boxes, one after the other, by the whole wave: every lane of the wave arrives here
    unsigned long long pending = __ballot(large);
    const int lx = threadIdx.x & 7, ly = (threadIdx.x >> 3) & 7;
    while (pending) {
        const int src = __ffsll((long long)pending) - 1;
        pending &= pending - 1;
        Tri s;
        s.X0 = __shfl(t.X0, src, 64); s.Y0 = __shfl(t.Y0, src, 64);
        s.X1 = __shfl(t.X1, src, 64); s.Y1 = __shfl(t.Y1, src, 64);
        s.X2 = __shfl(t.X2, src, 64); s.Y2 = __shfl(t.Y2, src, 64);
        s.d0 = __shfl(t.d0, src, 64); s.d1 = __shfl(t.d1, src, 64); s.d2 = __shfl(t.d2, src, 64);
        s.A2 = __shfl(t.A2, src, 64);
        const int sx0 = __shfl(bx0, src, 64), sy0 = __shfl(by0, src, 64), sw = __shfl(bw, src, 64), sh = __shfl(bh, src, 64);
        const double A2 = (double)s.A2;
        Edges e;
        edges_at(s, sx0 + lx, sy0 + ly, e);                 // this lane's sample of the first tile; then steps of 8 columns
        for (int ty = 0; ty < sh; ty += 8) {
            long long E0 = e.E0, E1 = e.E1, E2 = e.E2;
            const int y = ty + ly;
            for (int tx = 0; tx < sw; tx += 8) {
                const int x = tx + lx;
                if (x < sw && y < sh)
                    cross(E0, E1, E2, e.nb0, e.nb1, e.nb2, s.d0, s.d1, s.d2, A2, a, ca, sx0 + x, sy0 + y, L.cy, wz, grid);
                E0 += 8 * e.dx0; E1 += 8 * e.dx1; E2 += 8 * e.dx2;
            }
            e.E0 += 8 * e.dy0; e.E1 += 8 * e.dy1; e.E2 += 8 * e.dy2;
        }
    }
}

// prefix parity along x (AXIS 0) or y (AXIS 1): one thread per word column, a running XOR of whole words over the slabs
template <int AXIS>
__global__ __launch_bounds__(BLOCK) void voxel_prefix_xy_kernel(unsigned *__restrict__ grid, const int cx, const int cy, const int wz,
                                                               int *counters) {
    const int t = blockIdx.x * BLOCK + threadIdx.x;
    const int n = (AXIS == 0 ? cy : cx) * wz;
    if (t >= n) return;
    int first, stride, steps;
    if (AXIS == 0) {
        first = t;                                          // (iy, word) of slab ix = 0
        stride = cy * wz;
        steps = cx;
    } else {
        const int ix = t / wz;
        first = ix * cy * wz + (t - ix * wz);               // (ix, word) of row iy = 0
        stride = wz;
        steps = cy;
    }
    unsigned run = 0u;
    for (int s = 0; s < steps; ++s) {
        unsigned *p = grid + first + s * stride;
        run ^= *p;
        *p = run;
    }
    if (run) atomicAdd(counters + 2 + AXIS, __popc(run));   // no mark lies beyond cz: the padding bits are zero
}

// prefix parity along z: one thread per row, inside each word by shifts, the carry across the row's words
__global__ __launch_bounds__(BLOCK) void voxel_prefix_z_kernel(unsigned *__restrict__ grid, const int rows, const int wz, int *counters) {
    const int r = blockIdx.x * BLOCK + threadIdx.x;
    if (r >= rows) return;
    unsigned carry = 0u;
    for (int w = 0; w < wz; ++w) {
        unsigned v = grid[r * wz + w];
        v ^= v << 1;
        v ^= v << 2;
        v ^= v << 4;
        v ^= v << 8;
        v ^= v << 16;
        v ^= 0u - carry;
        carry = v >> 31;
        grid[r * wz + w] = v;
    }
    if (carry) atomicAdd(counters + 4, 1);                  // no mark lies beyond cz: the last bit is the column's total parity
}

// `take` bits of row r from bit iz on (iz + take <= 32 wz)
__device__ __forceinline__ unsigned row_bits(const unsigned *__restrict__ grid, int r, int wz, int iz) {
    const int q = iz >> 5, s = iz & 31;
    unsigned v = grid[r * wz + q] >> s;
    if (s != 0 && q + 1 < wz) v |= grid[r * wz + q + 1] << (32 - s);
    return v;
}

// one thread per output word: the row segments that make up its 32 cells, from one grid or the majority of three
__global__ __launch_bounds__(BLOCK) void voxel_combine_kernel(const unsigned *__restrict__ scratch, const int grid_words, const int axes,
                                                             const int rows, const int cz, const int wz, const int n_words,
                                                             unsigned *__restrict__ words) {
    const int w = blockIdx.x * BLOCK + threadIdx.x;
    if (w >= n_words) return;
    const long long l0 = 32ll * w;
    int r = (int)(l0 / cz), iz = (int)(l0 - (long long)r * cz);
    unsigned out = 0u;
    for (int pos = 0; pos < 32 && r < rows; ++r, iz = 0) {  // at most 32 segments
        const int take = min(32 - pos, cz - iz);
        unsigned v;
        if (axes == AXES_MAJORITY) {
            const unsigned p = row_bits(scratch, r, wz, iz), q = row_bits(scratch + grid_words, r, wz, iz),
                           s = row_bits(scratch + 2ll * grid_words, r, wz, iz);
            v = (p & q) | (p & s) | (q & s);
        } else {
            v = row_bits(scratch, r, wz, iz);
        }
        if (take < 32) v &= (1u << take) - 1u;
        out |= v << pos;
        pos += take;
    }
    words[w] = out;
}
#endif  // __HIPCC__

// ---- host side --------------------------------------------------------------------------------------------------------------
static inline bool lattice_from_args(const float *box, const int *cells, Lattice &L) {
    static const int some_words = 0;
    bitgrid::Grid g;
    if (!bitgrid::grid_from_args(box, cells, &some_words, g)) return false;
    L = Lattice{(double)g.bx, (double)g.by, (double)g.bz, (double)g.ix, (double)g.iy, (double)g.iz, g.cx, g.cy, g.cz};
    return true;
}
static inline bool mesh_ok(const float *verts, const int *faces, int64_t V, int64_t F) {
    if (V < 0 || V > INT_MAX64 || F < 0 || 3 * F > INT_MAX64) return false;
    return (V == 0 || verts) && (F == 0 || faces);
}
static inline bool axes_ok(int axes) { return axes >= 0 && axes <= AXES_MAJORITY; }
static inline int grid_words_of(const Lattice &L) { return L.cx * L.cy * words_per_row(L.cz); }      // <= 2^22

}  // namespace voxel
}  // namespace mvip

#ifndef MVIP_VOXEL_NO_ENTRY_POINTS
using namespace mvip;
namespace vx = mvip::voxel;

extern "C" int64_t mvip_voxel_scratch_words(const int *cells, int axes) {
    if (!cells || !bitgrid::cells_ok(cells[0], cells[1], cells[2]) || !vx::axes_ok(axes)) return -1;
    return (int64_t)(axes == vx::AXES_MAJORITY ? 3 : 1) * cells[0] * cells[1] * vx::words_per_row(cells[2]);
}

extern "C" int mvip_voxel_surface(const float *verts, const int *faces, int64_t n_verts, int64_t n_faces, const float *box,
                                  const int *cells, int *words, int *counters, void *stream) {
    vx::Lattice L;
    if (!vx::lattice_from_args(box, cells, L) || !vx::mesh_ok(verts, faces, n_verts, n_faces) || !words || !counters) return MVIP_EINVAL;
    hipStream_t s = as_stream(stream);
    const int n = bitgrid::n_words(L.cx, L.cy, L.cz);
    hipLaunchKernelGGL(vx::voxel_clear_kernel, dim3(blocks_for(n, vx::BLOCK)), dim3(vx::BLOCK), 0, s, (unsigned *)words, n, counters);
    if (n_faces > 0)                                        // with Nv = 0 every index is outside [0, 0): verts is never read
        hipLaunchKernelGGL(vx::voxel_surface_kernel, dim3(blocks_for(n_faces, vx::BLOCK)), dim3(vx::BLOCK), 0, s, verts, faces,
                           (int)n_verts, (int)n_faces, L, (unsigned *)words, counters);
    return check_launch();
}

extern "C" int mvip_voxel_crossings(const float *verts, const int *faces, int64_t n_verts, int64_t n_faces, const float *box,
                                    const int *cells, int axes, int *scratch, int *counters, void *stream) {
    vx::Lattice L;
    if (!vx::lattice_from_args(box, cells, L) || !vx::mesh_ok(verts, faces, n_verts, n_faces) || !vx::axes_ok(axes) || !scratch ||
        !counters)
        return MVIP_EINVAL;
    const int n_axes = axes == vx::AXES_MAJORITY ? 3 : 1;
    const int64_t blocks_per_axis = (n_faces + vx::BLOCK - 1) / vx::BLOCK;
    if (blocks_per_axis * n_axes > vx::INT_MAX64) return MVIP_EINVAL;
    hipStream_t s = as_stream(stream);
    const int gw = vx::grid_words_of(L);
    hipLaunchKernelGGL(vx::voxel_clear_kernel, dim3(blocks_for((int64_t)n_axes * gw, vx::BLOCK)), dim3(vx::BLOCK), 0, s,
                       (unsigned *)scratch, n_axes * gw, counters);
    if (n_faces > 0)                                        // with Nv = 0 every index is outside [0, 0): verts is never read
        hipLaunchKernelGGL(vx::voxel_crossings_kernel, dim3((unsigned)(blocks_per_axis * n_axes)), dim3(vx::BLOCK), 0, s, verts, faces,
                           (int)n_verts, (int)n_faces, L, axes, (int)blocks_per_axis, gw, (unsigned *)scratch, counters);
    return check_launch();
}

extern "C" int mvip_voxel_fill(int *scratch, const int *cells, int axes, int *words, int *counters, void *stream) {
    if (!cells || !bitgrid::cells_ok(cells[0], cells[1], cells[2]) || !vx::axes_ok(axes) || !scratch || !words || !counters)
        return MVIP_EINVAL;
    hipStream_t s = as_stream(stream);
    const int cx = cells[0], cy = cells[1], cz = cells[2], wz = vx::words_per_row(cz), gw = cx * cy * wz;
    unsigned *g = (unsigned *)scratch;
    const dim3 block(vx::BLOCK);
    if (axes == 0 || axes == vx::AXES_MAJORITY)
        hipLaunchKernelGGL(vx::voxel_prefix_xy_kernel<0>, dim3(blocks_for(cy * wz, vx::BLOCK)), block, 0, s, g, cx, cy, wz, counters);
    if (axes == 1 || axes == vx::AXES_MAJORITY)
        hipLaunchKernelGGL(vx::voxel_prefix_xy_kernel<1>, dim3(blocks_for(cx * wz, vx::BLOCK)), block, 0, s,
                           g + (axes == vx::AXES_MAJORITY ? gw : 0), cx, cy, wz, counters);
    if (axes == 2 || axes == vx::AXES_MAJORITY)
        hipLaunchKernelGGL(vx::voxel_prefix_z_kernel, dim3(blocks_for(cx * cy, vx::BLOCK)), block, 0, s,
                           g + (axes == vx::AXES_MAJORITY ? 2 * gw : 0), cx * cy, wz, counters);
    const int n = bitgrid::n_words(cx, cy, cz);
    hipLaunchKernelGGL(vx::voxel_combine_kernel, dim3(blocks_for(n, vx::BLOCK)), block, 0, s, (const unsigned *)g, gw, axes, cx * cy, cz,
                       wz, n, (unsigned *)words);
    return check_launch();
}
#endif  // MVIP_VOXEL_NO_ENTRY_POINTS
