"""Mesh topology timings (profiles/mesh_topology.json): ops.mesh_edge_table, mesh_components ('edge' and 'vertex'),
mesh_boundary_loops and mesh_cap_loops (csrc/mesh_topology.hip) on the marching-cubes mesh of the 4-period gyroid at 256^3 (2.5 M
triangles, the mesh of tools/mesh_ops_bench.py), each as the API call with its allocations and read-backs; beside them the
corner table of the same mesh on preallocated buffers (the yardstick: tools/mesh_ops_bench.py's ms_corner_table) and the
kernels of the edge table alone.  HIP-event times, the median of 5 windows after a warm-up.  Then the gyroid's topology
report, and what mesh.drop_interior(32 directions) followed by keep_components(largest=1) and close_holes does to it.  The
loop and cap operations are timed on the mesh after drop_interior as well: the closed gyroid has no boundary to walk.  A
record, not a gate.

  python tools/mesh_topology_bench.py [--out profile_out/mesh_topology.json] [--size 256] [--commit HASH]
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
from tools.mesh_ops_bench import lists_fn                            # noqa: E402

I32 = torch.int32
LO, HI = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)


def edge_kernels_fn(f, V):
    """the launches of the edge table on preallocated buffers: keys, the lo-lists, the walk with its ranks, the emit pass (at the
    edge count of a first run)."""
    F, dev = int(f.shape[0]), f.device
    n = 3 * F
    e = lambda *s: torch.empty(s, device=dev, dtype=I32)
    keys, flag, rep, hc, hf, twin, rank, edge_of = e(n), e(1), e(n), e(n), e(n), e(n), e(n), e(n)
    wg = e(max(1, _lib.load().mvip_mesh_rank_groups(n)))
    total = torch.empty(1, device=dev, dtype=torch.int64)
    E = int(ops.mesh_edge_table(f, V).first.shape[0])
    edges, first, count, forward = e(E, 2), e(E), e(E), e(E)
    offsets, items = e(V + 1), e(n)
    scratch = e(_lib.load().mvip_mesh_list_scratch_words(n, V))
    lflag = e(1)
    p = lambda t: ptr(t, I32)

    def run():
        st = stream()
        call('mvip_mesh_topology_keys', p(f), F, V, p(keys), p(flag), st)
        call('mvip_mesh_corner_table', p(keys), n, V, p(offsets), p(items), p(scratch), p(lflag), st)
        call('mvip_mesh_topology_edges_find', p(f), F, V, p(keys), p(offsets), p(items), p(rep), p(hc), p(hf), p(twin), p(wg), p(rank),
             ptr(total, torch.int64), st)
        call('mvip_mesh_topology_edges_emit', p(f), F, p(rep), p(hc), p(hf), p(rank), E, p(edge_of), p(edges), p(first), p(count),
             p(forward), st)
    return run


def timings(m):
    v, f = m.verts, m.faces
    V = int(v.shape[0])
    ms = lambda fn: round(event_ms(fn, warmup=1, reps=5)[0], 4)
    return {
        'ms_corner_table_kernels': ms(lists_fn(f.reshape(-1), V)),
        'ms_edge_table_kernels': ms(edge_kernels_fn(f, V)),
        'ms_api_mesh_edge_table': ms(lambda: ops.mesh_edge_table(f, V)),
        'ms_api_mesh_components_edge': ms(lambda: ops.mesh_components(f, V, 'edge')),
        'ms_api_mesh_components_vertex': ms(lambda: ops.mesh_components(f, V, 'vertex')),
        'ms_api_mesh_boundary_loops': ms(lambda: ops.mesh_boundary_loops(f, V)),
        'ms_api_mesh_cap_loops_64': ms(lambda: ops.mesh_cap_loops(v, f, None, 64)),
    }


def report(m):
    rep = mesh.topology(m)
    rep['largest_components_faces'] = sorted((c['faces'] for c in rep.pop('per_component')), reverse=True)[:8]
    sizes = mesh.boundary_loops(m).sizes
    rep['largest_loops'] = sorted(sizes.tolist(), reverse=True)[:8]
    return rep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--commit', default='')
    a = ap.parse_args()
    dev = torch.device('cuda', 0)
    a.out = a.out or os.path.join(ROOT, 'profile_out', 'mesh_topology.json')
    n = a.size
    v, f, normals = mesh.marching_cubes(gyroid(n, dev), 1.5, LO, HI)
    m = mesh.Mesh(v, f, normals, None)
    out = {'commit': a.commit, 'device': torch.cuda.get_device_name(0), 'mesh': 'gyroid, 4 periods, iso 1.5', 'grid': [n, n, n],
           'vertices': int(v.shape[0]), 'triangles': int(f.shape[0]), 'timings': timings(m), 'report': report(m)}
    cut = mesh.drop_interior(m, directions=32)
    kept = mesh.keep_components(cut, largest=1)
    closed, capped, left = mesh.close_holes(kept, max_edges=64)
    out['after_drop_interior_32'] = {'timings': timings(cut), 'report': report(cut)}
    out['then_keep_components_largest_1'] = {'report': report(kept)}
    out['then_close_holes_64'] = {'loops_capped': capped, 'loops_left': left, 'report': report(closed)}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out))
    return 0


if __name__ == '__main__':
    sys.exit(main())
