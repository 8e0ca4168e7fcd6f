// A stand-alone HOST program that walks the __host__ __device__ functions of csrc/mesh_voxel.hip -- lattice coordinates, the
// guard band, the snapped integer set-up, coverage, the crossing cell, the candidate range, the triangle-box overlap -- over the
// cases of a file that tests/test_voxel_host.py writes from the numpy restatement, and compares bit for bit.  No GPU is touched:
// the faces are walked in a plain loop, the parity prefix and the majority are taken cell by cell.  Meant to be compiled with
// the host sanitizers (hipcc -Xarch_host -fsanitize=address,undefined), so that an out-of-range index or an overflowing
// conversion in the shared functions shows before a kernel first runs.
//
// File: int32 n_cases, then per case int32 Nv, F, cx, cy, cz; fp32 box[6]; fp32 verts[3 Nv]; int32 faces[3 F]; for axes = 0..3
// int32 words[n], odd[3], dropped; then the surface's int32 words[n], dropped.  Exit status 0: every case equal.
#define MVIP_VOXEL_NO_ENTRY_POINTS
#include "../mvip_nerf_amd/csrc/mesh_voxel.hip"

#include <cstdio>
#include <vector>

namespace mvip {
void set_last_error(hipError_t) {}
}

using namespace mvip::voxel;

template <class T>
static bool get(FILE *f, std::vector<T> &v, size_t n) {
    v.resize(n);
    return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

struct Case {
    int Nv, F, cx, cy, cz;
    std::vector<float> box, verts;
    std::vector<int> faces;
};

static bool index_ok(const Case &c, int fi) {
    for (int k = 0; k < 3; ++k)
        if ((unsigned)c.faces[3 * fi + k] >= (unsigned)c.Nv) return false;
    return true;
}

static Lattice lattice_of(const Case &c) {
    return Lattice{(double)c.box[0], (double)c.box[1], (double)c.box[2], (double)c.box[3], (double)c.box[4], (double)c.box[5], c.cx, c.cy, c.cz};
}

static void solid(const Case &c, int axes, std::vector<int> &words, int odd[3], int &dropped) {
    const Lattice L = lattice_of(c);
    const int wz = words_per_row(c.cz), gw = c.cx * c.cy * wz;
    const int n_axes = axes == AXES_MAJORITY ? 3 : 1;
    std::vector<unsigned> scratch((size_t)n_axes * gw, 0u);
    dropped = 0;
    for (int slot = 0; slot < n_axes; ++slot) {
        const int a = axes == AXES_MAJORITY ? slot : axes;
        const int b = a == 2 ? 0 : a + 1, cc = b == 2 ? 0 : b + 1;
        const int ca = sel(a, L.cx, L.cy, L.cz), cb = sel(b, L.cx, L.cy, L.cz), ccn = sel(cc, L.cx, L.cy, L.cz);
        for (int fi = 0; fi < c.F; ++fi) {
            if (!index_ok(c, fi)) continue;
            Face f;
            lattice_face(L, c.verts.data(), c.faces[3 * fi], c.faces[3 * fi + 1], c.faces[3 * fi + 2], f);
            if (!face_kept(f, axes)) {
                dropped += slot == 0;
                continue;
            }
            Tri t;
            int x0, y0, w, h;
            if (!setup(f, a, t) || !sample_box(t, cb, ccn, x0, y0, w, h)) continue;
            Edges e;
            edges_at(t, x0, y0, e);
            for (int y = 0; y < h; ++y) {
                long long E0 = e.E0, E1 = e.E1, E2 = e.E2;
                for (int x = 0; x < w; ++x) {
                    const int k = crossing_cell(E0, E1, E2, e.nb0, e.nb1, e.nb2, t.d0, t.d1, t.d2, (double)t.A2, ca);
                    if (k >= 0) {
                        int word;
                        unsigned bit;
                        crossing_bit(a, x0 + x, y0 + y, k, L.cy, wz, word, bit);
                        scratch.at((size_t)slot * gw + word) ^= bit;
                    }
                    E0 += e.dx0; E1 += e.dx1; E2 += e.dx2;
                }
                e.E0 += e.dy0; e.E1 += e.dy1; e.E2 += e.dy2;
            }
        }
    }
    // the prefix parity and the majority, cell by cell
    auto crossing = [&](int slot, int ix, int iy, int iz) { return (scratch[(size_t)slot * gw + (ix * c.cy + iy) * wz + (iz >> 5)] >> (iz & 31)) & 1u; };
    const int dims[3] = {c.cx, c.cy, c.cz};
    std::vector<unsigned char> votes((size_t)c.cx * c.cy * c.cz, 0);
    odd[0] = odd[1] = odd[2] = 0;
    for (int slot = 0; slot < n_axes; ++slot) {
        const int a = axes == AXES_MAJORITY ? slot : axes;
        const int b = (a + 1) % 3, cc = (a + 2) % 3;
        for (int x = 0; x < dims[b]; ++x)
            for (int y = 0; y < dims[cc]; ++y) {
                unsigned run = 0u;
                for (int k = 0; k < dims[a]; ++k) {
                    int i[3];
                    i[a] = k; i[b] = x; i[cc] = y;
                    run ^= crossing(slot, i[0], i[1], i[2]);
                    votes[((size_t)i[0] * c.cy + i[1]) * c.cz + i[2]] += run;
                }
                odd[a] += run;
            }
    }
    const size_t n = votes.size();
    words.assign((n + 31) / 32, 0);
    for (size_t l = 0; l < n; ++l)
        if (votes[l] >= (axes == AXES_MAJORITY ? 2 : 1)) words[l >> 5] |= (int)(1u << (l & 31));
}

static void surface(const Case &c, std::vector<int> &words, int &dropped) {
    const Lattice L = lattice_of(c);
    const size_t n = (size_t)c.cx * c.cy * c.cz;
    words.assign((n + 31) / 32, 0);
    dropped = 0;
    for (int fi = 0; fi < c.F; ++fi) {
        if (!index_ok(c, fi)) continue;
        Face f;
        lattice_face(L, c.verts.data(), c.faces[3 * fi], c.faces[3 * fi + 1], c.faces[3 * fi + 2], f);
        if (!face_finite(f)) {
            ++dropped;
            continue;
        }
        int x0, y0, z0, nx, ny, nz;
        if (!candidate_range(f.x0, f.x1, f.x2, L.cx, x0, nx) || !candidate_range(f.y0, f.y1, f.y2, L.cy, y0, ny) ||
            !candidate_range(f.z0, f.z1, f.z2, L.cz, z0, nz))
            continue;
        for (int ix = x0; ix < x0 + nx; ++ix)
            for (int iy = y0; iy < y0 + ny; ++iy)
                for (int iz = z0; iz < z0 + nz; ++iz)
                    if (overlaps(f, ix, iy, iz)) {
                        const size_t l = ((size_t)ix * L.cy + iy) * L.cz + iz;
                        words.at(l >> 5) |= (int)(1u << (l & 31));
                    }
    }
}

int main(int argc, char **argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: %s cases.bin\n", argv[0]);
        return 2;
    }
    FILE *fp = fopen(argv[1], "rb");
    int n_cases = 0;
    if (!fp || fread(&n_cases, 4, 1, fp) != 1) {
        fprintf(stderr, "cannot read %s\n", argv[1]);
        return 2;
    }
    int bad = 0;
    for (int i = 0; i < n_cases; ++i) {
        Case c;
        int head[5];
        if (fread(head, 4, 5, fp) != 5) return 2;
        c.Nv = head[0]; c.F = head[1]; c.cx = head[2]; c.cy = head[3]; c.cz = head[4];
        if (!get(fp, c.box, 6) || !get(fp, c.verts, 3 * (size_t)c.Nv) || !get(fp, c.faces, 3 * (size_t)c.F)) return 2;
        const size_t n = ((size_t)c.cx * c.cy * c.cz + 31) / 32;
        std::vector<int> want, got, tail;
        for (int axes = 0; axes <= AXES_MAJORITY; ++axes) {
            if (!get(fp, want, n) || !get(fp, tail, 4)) return 2;
            int odd[3], dropped;
            solid(c, axes, got, odd, dropped);
            const bool ok = got == want && odd[0] == tail[0] && odd[1] == tail[1] && odd[2] == tail[2] && dropped == tail[3];
            if (!ok) {
                size_t diff = 0;
                for (size_t w = 0; w < n; ++w) diff += (size_t)__builtin_popcount((unsigned)(got[w] ^ want[w]));
                printf("case %d axes %d: %zu bits differ, odd %d %d %d (want %d %d %d), dropped %d (want %d)\n", i, axes, diff, odd[0], odd[1],
                       odd[2], tail[0], tail[1], tail[2], dropped, tail[3]);
                ++bad;
            }
        }
        if (!get(fp, want, n) || !get(fp, tail, 1)) return 2;
        int dropped;
        surface(c, got, dropped);
        if (got != want || dropped != tail[0]) {
            printf("case %d surface differs, dropped %d (want %d)\n", i, dropped, tail[0]);
            ++bad;
        }
    }
    fclose(fp);
    printf("%d cases, %d mismatches\n", n_cases, bad);
    return bad ? 1 : 0;
}
