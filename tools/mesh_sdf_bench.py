"""Signed mesh distance timings (profiles/mesh_sdf.json; csrc/mesh_sdf.hip) on the marching-cubes mesh of the 4-period gyroid of
tools/mesh_ops_bench.py (256^3: 2.5 M triangles), the mesh of tools/mesh_distance_bench.py.

  pseudonormals: ops.mesh_vertex_pseudonormals whole (the corner table and the kernel) and the kernel's share of it.
  query: ops.mesh_signed_distance on that tool's near-surface queries (4 samples per face of the mesh clustered at 2 lattice
    steps, face-major) with grid, twin and pseudonormals given, beside ops.mesh_closest_point on the same queries with the same
    grid in the same process: both times and their ratio; the point-face tests per query of the counting variant.
  lattice: ops.mesh_signed_distance_lattice at --lattice^3 points with a band of 3 lattice steps: the time, the in-band share,
    the point-face tests per lattice point, and the same lattice without a band at --lattice-free^3 (a smaller one: every point
    then walks until it has found the surface).
  remesh: mesh.remesh end to end at --lattice points per axis, and the triangles it gives.

HIP-event times, the median of 5 windows after a warm-up; `kernels` holds the register counts of tools/kernel_regs.py, which
reads the build's object files: where those are not at hand (a machine that received only the library) the list is empty and
`python tools/kernel_regs.py mesh_sdf` on the build machine fills it.

  python tools/mesh_sdf_bench.py [--size 256] [--lattice 256] [--lattice-free 128] [--out profiles/mesh_sdf.json] [--commit HASH]
"""
import argparse
import json
import os
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from mvip_nerf_amd import mesh, ops                                  # noqa: E402
from tools.mesh_bench import event_ms, gyroid                        # noqa: E402

LO, HI = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)


def kernel_rows():
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'kernel_regs.py'), 'mesh_sdf'], capture_output=True, text=True)
    return [' '.join(line.split()) for line in r.stdout.split('\n') if 'meshsdf' in line]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--lattice', type=int, default=256)
    ap.add_argument('--lattice-free', type=int, default=128)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'mesh_sdf.json'))
    ap.add_argument('--commit', default='')
    a = ap.parse_args()
    dev = torch.device('cuda', 0)
    v, f, _ = mesh.marching_cubes(gyroid(a.size, dev), 1.5, LO, HI)
    V, F = int(v.shape[0]), int(f.shape[0])
    h = 2.0 / (a.size - 1)
    out = {'commit': a.commit, 'device': torch.cuda.get_device_name(0), 'mesh': f'gyroid, 4 periods, iso 1.5, {a.size}^3', 'vertices': V,
           'triangles': F, 'kernels': kernel_rows()}

    offsets, corners = ops.mesh_corner_table(f, V)
    P = torch.empty((V, 3), device=dev, dtype=torch.float64)
    from mvip_nerf_amd._lib import call, ptr, stream
    t_kernel, _ = event_ms(lambda: call('mvip_mesh_vertex_pseudonormals', ptr(v), ptr(f, torch.int32), V, F, ptr(offsets, torch.int32),
                                        ptr(corners, torch.int32), ptr(P, torch.float64), stream()))
    t_api, reps = event_ms(lambda: ops.mesh_vertex_pseudonormals(v, f))
    out['pseudonormals'] = {'ms_api_mesh_vertex_pseudonormals': round(t_api, 4), 'ms_reps': [round(t, 4) for t in reps],
                            'ms_kernel_alone': round(t_kernel, 4), 'vertices_per_second_kernel': round(V / (t_kernel * 1e-3))}
    t_twin, _ = event_ms(lambda: ops.mesh_edge_table(f, V), warmup=1, reps=3)
    out['ms_api_mesh_edge_table'] = round(t_twin, 4)
    twin, P, g = ops.mesh_edge_table(f, V).twin, ops.mesh_vertex_pseudonormals(v, f), ops.mesh_face_grid(v, f)

    cv, cf, _, _ = ops.mesh_cluster(v, f, None, None, 2 * h, 'quadric')
    pts = ops.mesh_sample_faces(cv, cf, 2)[0]
    N = int(pts.shape[0])
    kw = dict(grid=g, twin=twin, pseudonormals=P)
    t_closest, reps_c = event_ms(lambda: ops.mesh_closest_point(pts, v, f, grid=g))
    t_signed, reps_s = event_ms(lambda: ops.mesh_signed_distance(pts, v, f, **kw))
    t_closest2, _ = event_ms(lambda: ops.mesh_closest_point(pts, v, f, grid=g))          # again, after: the order of the two is not it
    sd, face, point, stats = ops.mesh_signed_distance(pts, v, f, return_stats=True, **kw)
    cface, cpoint, cdist = ops.mesh_closest_point(pts, v, f, grid=g)
    tests = int(stats.cpu()[0])
    out['query'] = {'queries': N, 'ms_mesh_signed_distance': round(t_signed, 4), 'ms_reps_signed': [round(t, 4) for t in reps_s],
                    'ms_mesh_closest_point': round(t_closest, 4), 'ms_reps_closest': [round(t, 4) for t in reps_c],
                    'ms_mesh_closest_point_again': round(t_closest2, 4), 'signed_over_closest': round(t_signed / t_closest, 4),
                    'point_face_tests_per_query': round(tests / N, 2), 'negative_share': round(float((sd < 0).float().mean()), 4),
                    'equal_to_mesh_closest_point': bool(torch.equal(face, cface) and torch.equal(point, cpoint) and torch.equal(sd.abs(), cdist))}

    n = a.lattice
    step = float(max(ops.mesh_lattice(LO, HI, n)[1]))
    band = 3 * step
    t_lat, reps_l = event_ms(lambda: ops.mesh_signed_distance_lattice(v, f, LO, HI, n, max_dist=band, **kw))
    _, lface, stats = ops.mesh_signed_distance_lattice(v, f, LO, HI, n, max_dist=band, return_stats=True, **kw)
    tests, slots = (int(x) for x in stats.cpu())
    out['lattice'] = {'points_per_axis': n, 'band_in_steps': 3, 'ms_mesh_signed_distance_lattice': round(t_lat, 4),
                      'ms_reps': [round(t, 4) for t in reps_l], 'points_per_second': round(n ** 3 / (t_lat * 1e-3)),
                      'in_band_share': round(float((lface >= 0).float().mean()), 4), 'point_face_tests_per_point': round(tests / n ** 3, 2),
                      'lane_utilisation_of_the_face_loop': round(tests / max(slots, 1), 4)}
    del lface
    m = a.lattice_free
    t_free, _ = event_ms(lambda: ops.mesh_signed_distance_lattice(v, f, LO, HI, m, **kw), warmup=1, reps=3)
    _, _, stats = ops.mesh_signed_distance_lattice(v, f, LO, HI, m, return_stats=True, **kw)
    out['lattice_without_band'] = {'points_per_axis': m, 'ms_mesh_signed_distance_lattice': round(t_free, 4),
                                   'points_per_second': round(m ** 3 / (t_free * 1e-3)),
                                   'point_face_tests_per_point': round(int(stats.cpu()[0]) / m ** 3, 2)}

    src = mesh.Mesh(v, f, None, None)
    box = {}
    t_re, reps_r = event_ms(lambda: box.__setitem__('m', mesh.remesh(src, resolution=n, bound_min=LO, bound_max=HI)), warmup=1, reps=3)
    rm = box['m']
    out['remesh'] = {'points_per_axis': n, 'ms_mesh_remesh': round(t_re, 4), 'ms_reps': [round(t, 4) for t in reps_r],
                     'triangles': int(rm.faces.shape[0]), 'vertices': int(rm.verts.shape[0]),
                     'largest_distance_to_the_input_in_steps': round(float(ops.mesh_closest_point(rm.verts, v, f, grid=g)[2].max()) / step, 4)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out), flush=True)
    return 0


if __name__ == '__main__':
    sys.exit(main())
