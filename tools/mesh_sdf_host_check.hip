// A stand-alone HOST program that walks the __host__ __device__ functions of csrc/mesh_distance_device.h and csrc/mesh_sdf.hip --
// point_triangle with its feature code, the face normals, the pseudonormal of the closest feature, the sign -- over the cases
// of a file that tests/test_mesh_sdf_host.py writes from the numpy restatement, and compares bit for bit.  No GPU is touched:
// every query is taken against every face in a plain loop (the smallest d2, the lowest face among equals), which is what the
// kernel's walk over the face grid must equal.  Meant to be compiled with the host sanitizers (hipcc -Xarch_host
// -fsanitize=address,undefined), so that an out-of-range index in the shared functions shows before a kernel first runs.
// The vertex pseudonormals P come from the file: their atan2 is the one operation that is not pinned bit for bit.
//
// File: int32 n_cases, then per case int32 Nv, F, N; fp32 verts[3 Nv]; int32 faces[3 F]; int32 twin[3 F]; fp64 P[3 Nv];
// fp32 points[3 N]; then the expected int32 face[N], int32 feature[N], fp32 sdist[N], fp32 point[3 N].  Exit status 0: equal.
#define MVIP_MESH_SDF_NO_ENTRY_POINTS
#include "../mvip_nerf_amd/csrc/mesh_sdf.hip"

#include <cstdio>
#include <cstring>
#include <vector>

namespace mvip {
void set_last_error(hipError_t) {}
}

using namespace mvip::meshdist;
using namespace mvip::meshsdf;

template <class T>
static bool get(FILE *f, std::vector<T> &v, size_t n) {
    v.resize(n);
    return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

static bool same_bits(float a, float b) { return memcmp(&a, &b, 4) == 0 || (a != a && b != b); }

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
    long long queries = 0;
    for (int i = 0; i < n_cases; ++i) {
        int head[3];
        if (fread(head, 4, 3, fp) != 3) return 2;
        const int Nv = head[0], F = head[1], N = head[2];
        std::vector<float> verts, points, want_sd, want_point;
        std::vector<int> faces, twin, want_face, want_feat;
        std::vector<double> P;
        if (!get(fp, verts, 3 * (size_t)Nv) || !get(fp, faces, 3 * (size_t)F) || !get(fp, twin, 3 * (size_t)F) ||
            !get(fp, P, 3 * (size_t)Nv) || !get(fp, points, 3 * (size_t)N) || !get(fp, want_face, (size_t)N) ||
            !get(fp, want_feat, (size_t)N) || !get(fp, want_sd, (size_t)N) || !get(fp, want_point, 3 * (size_t)N))
            return 2;
        int wrong = 0;
        for (int n = 0; n < N; ++n) {
            const float fx = points[3 * n], fy = points[3 * n + 1], fz = points[3 * n + 2];
            const float nan = __builtin_nanf("");
            float sd = nan, q[3] = {nan, nan, nan};
            int bf = -1, feat = -1;
            if (mvip::finite(fx) && mvip::finite(fy) && mvip::finite(fz)) {
                const double px = (double)fx, py = (double)fy, pz = (double)fz;
                double best = __builtin_huge_val(), bq[3] = {0.0, 0.0, 0.0};
                for (int f = 0; f < F; ++f) {
                    double d2, qx, qy, qz;
                    int ft;
                    if (!point_face(verts.data(), faces.data(), Nv, f, px, py, pz, d2, qx, qy, qz, ft)) continue;
                    if (d2 < best) {                          // ascending f: strict keeps the lowest face among equals
                        best = d2;
                        bf = f;
                        feat = ft;
                        bq[0] = qx; bq[1] = qy; bq[2] = qz;
                    }
                }
                if (bf >= 0) {
                    sd = (float)sqrt(best);
                    if (best > 0.0 && sign_negative(verts.data(), faces.data(), Nv, F, twin.data(), P.data(), bf, feat, px, py, pz,
                                                    bq[0], bq[1], bq[2]))
                        sd = -sd;
                    for (int a = 0; a < 3; ++a) q[a] = (float)bq[a];
                }
            }
            const bool ok = bf == want_face[n] && feat == want_feat[n] && same_bits(sd, want_sd[n]) && same_bits(q[0], want_point[3 * n]) &&
                            same_bits(q[1], want_point[3 * n + 1]) && same_bits(q[2], want_point[3 * n + 2]);
            if (!ok && wrong++ < 5)
                printf("case %d query %d: face %d (want %d) feature %d (want %d) sdist %.9g (want %.9g)\n", i, n, bf, want_face[n], feat,
                       want_feat[n], sd, want_sd[n]);
        }
        bad += wrong;
        queries += N;
    }
    fclose(fp);
    printf("%d cases, %lld queries, %d mismatches\n", n_cases, queries, bad);
    return bad ? 1 : 0;
}
