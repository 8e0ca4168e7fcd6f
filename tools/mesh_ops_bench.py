"""Mesh clean-up timings (profiles/mesh_ops.json): the corner table, the vertex normals, one Taubin iteration and vertex
clustering at 2, 4 and 8 lattice steps (csrc/mesh_ops.hip) on the marching-cubes mesh of the analytic sphere (radius 0.6) at
256^3 and of the 4-period gyroid at 256^3 (2.5 M triangles, the size of the scene-1 sigma = 10 surface).  HIP-event times,
the median of 5 windows after a warm-up.  The corner table, the normals and the smoothing iteration run on preallocated
buffers (kernels only); clustering is the API call ops.mesh_cluster, with its allocations and its four read-backs, and
beside it the kernels of its two cluster lists alone.  With each clustering: triangles and vertices before and after, the
share of clusters the quadric placed, and the largest distance from an input vertex to its cluster's representative in
units of the cell (at most sqrt(3)).  A record, not a gate.

Bytes per corner and pass (F faces, V ~ F / 2 vertices, 3 F corners): the corner table reads each key three times (count,
fill, rank: 12 B) and writes / reads the unsorted and the sorted entry (4 + 4 L + 4 B for a list of length L, the L reads from
cache); normals read per corner 4 B of the table, 12 B of face indices and 36 B of positions (cached: each vertex is read ~18
times), smoothing 4 + 8 + 24 B; both write 12 B per vertex.

  python tools/mesh_ops_bench.py [--out profile_out/mesh_ops.json] [--sizes 256] [--commit HASH]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from mvip_nerf_amd import _lib, mesh, ops                            # noqa: E402
from mvip_nerf_amd._lib import ptr, stream, call                     # noqa: E402
from tools.mesh_bench import event_ms, gyroid                        # noqa: E402

I32 = torch.int32
LO, HI = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)


def sphere(n, dev, r=0.6):
    xs = mesh.grid_axes(LO, HI, n, dev)
    d = torch.sqrt(xs[0][:, None, None] ** 2 + xs[1][None, :, None] ** 2 + xs[2][None, None, :] ** 2)
    return (2.0 - d / r).contiguous()


def lists_fn(keys, n_lists):
    """the launches of one list build on preallocated buffers."""
    n = keys.shape[0]
    dev = keys.device
    offsets = torch.empty(n_lists + 1, device=dev, dtype=I32)
    items = torch.empty(n, device=dev, dtype=I32)
    scratch = torch.empty(_lib.load().mvip_mesh_list_scratch_words(n, n_lists), device=dev, dtype=I32)
    flag = torch.empty(1, device=dev, dtype=I32)
    return lambda: call('mvip_mesh_corner_table', ptr(keys, I32), n, n_lists, ptr(offsets, I32), ptr(items, I32),
                        ptr(scratch, I32), ptr(flag, I32), stream())


def row(name, grid, iso, n, dev):
    v, f, _ = mesh.marching_cubes(grid, iso, LO, HI)
    V, F = int(v.shape[0]), int(f.shape[0])
    h = 2.0 / (n - 1)
    off, cor = ops.mesh_corner_table(f, V)
    normals = torch.empty_like(v)
    a, b = v.clone(), torch.empty_like(v)

    def smooth_iteration():
        call('mvip_mesh_smooth_pass', ptr(a), ptr(f, I32), V, F, ptr(off, I32), ptr(cor, I32), 0.5, ptr(b), stream())
        call('mvip_mesh_smooth_pass', ptr(b), ptr(f, I32), V, F, ptr(off, I32), ptr(cor, I32), -0.53, ptr(a), stream())

    t_table, reps_table = event_ms(lists_fn(f.reshape(-1), V))
    t_normals, _ = event_ms(lambda: call('mvip_mesh_vertex_normals', ptr(v), ptr(f, I32), V, F, ptr(off, I32), ptr(cor, I32),
                                         ptr(normals), stream()))
    t_smooth, _ = event_ms(smooth_iteration)
    t_api_normals, _ = event_ms(lambda: ops.mesh_vertex_normals(v, f), warmup=1, reps=5)
    r = {'mesh': name, 'grid': [n, n, n], 'vertices': V, 'triangles': F, 'longest_corner_list': int((off[1:] - off[:-1]).max()),
         'ms_corner_table': round(t_table, 4), 'ms_corner_table_reps': [round(t, 4) for t in reps_table],
         'ms_vertex_normals': round(t_normals, 4), 'ms_smooth_iteration_two_passes': round(t_smooth, 4),
         'ms_api_mesh_vertex_normals': round(t_api_normals, 4), 'clustering': []}
    for steps in (2, 4, 8):
        cell = steps * h
        out = {}

        def cluster():
            out['r'] = ops.mesh_cluster(v, f, None, None, cell, 'quadric')
        t_cluster, reps = event_ms(cluster, warmup=1, reps=5)
        cv, cf, _, cov = out['r']
        t_mean, _ = event_ms(lambda: ops.mesh_cluster(v, f, None, None, cell, 'mean'), warmup=1, reps=5)
        mv = ops.mesh_cluster(v, f, None, None, cell, 'mean')[0]
        ok = cov >= 0
        disp = float((cv[cov[ok].long()] - v[ok]).norm(dim=1).max()) / cell
        # the two cluster lists alone (members by vertex, corners by remapped face), on the clusters before the drop
        cov0 = torch.unique(cov[ok], return_inverse=True)[1].to(I32).contiguous() if bool(ok.all()) else None
        t_lists = None
        if cov0 is not None:
            K = int(cov0.max()) + 1
            rf = cov0[f.reshape(-1).long()].contiguous()
            t_members, _ = event_ms(lists_fn(cov0, K))
            t_corners, _ = event_ms(lists_fn(rf, K))
            t_lists = {'ms_member_lists': round(t_members, 4), 'ms_corner_lists': round(t_corners, 4),
                       'longest_corner_list': int(torch.bincount(rf.long()).max())}
        r['clustering'].append({'lattice_steps': steps, 'cell': cell, 'ms_api_mesh_cluster_quadric': round(t_cluster, 4),
                                'ms_reps': [round(t, 4) for t in reps], 'ms_api_mesh_cluster_mean': round(t_mean, 4),
                                'triangles_after': int(cf.shape[0]), 'vertices_after': int(cv.shape[0]),
                                'triangle_ratio': round(cf.shape[0] / F, 4),
                                'share_placed_by_quadric': round(float((cv != mv).any(dim=1).float().mean()), 4),
                                'max_vertex_displacement_in_cells': round(disp, 4), 'lists': t_lists})
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--sizes', type=int, nargs='+', default=[256])
    ap.add_argument('--commit', default='')
    a = ap.parse_args()
    dev = torch.device('cuda', 0)
    a.out = a.out or os.path.join(ROOT, 'profile_out', 'mesh_ops.json')
    rows = []
    for n in a.sizes:
        rows.append(row('analytic sphere, radius 0.6, iso 1', sphere(n, dev), 1.0, n, dev))
        rows.append(row('gyroid, 4 periods, iso 1.5', gyroid(n, dev), 1.5, n, dev))
    out = {'commit': a.commit, 'device': torch.cuda.get_device_name(0), 'rows': rows}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))
    return 0


if __name__ == '__main__':
    sys.exit(main())
