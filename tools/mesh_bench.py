"""Mesh-export timings (profiles/mesh_extract.json): marching cubes alone (csrc/mcubes.hip) at 256^3 and 512^3 on an
analytic field, and the density query of mesh.density_grid at 256^3 for both models (8x256 MLP in exact fp32 and split
precision; the hash-grid model, whose fused kernel is exact fp32 only).  Times are HIP-event times of steady-state
repeats after a warm-up.

Bytes of the marching-cubes passes (compulsory traffic, N points, V vertices, F triangles): classify reads the grid and
writes one uint16 per point (6 N), the vertex pass reads those and writes an int32 first-vertex id (6 N) plus 24 B per
vertex, the triangle pass reads the uint16 again (2 N) plus 12 B per triangle: 14 N + 24 V + 12 F.  Neighbour reads of
the grid / of the id array are counted as cache hits.

  python tools/mesh_bench.py [--out profile_out/mesh_extract.json] [--commit HASH]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from mvip_nerf_amd import _lib, mesh, run                           # noqa: E402
from mvip_nerf_amd._lib import ptr, stream, call                     # noqa: E402
from tools.extract_mesh import model_args                            # noqa: E402

HBM_BYTES_PER_S = 6.3e12
MLP_FLOP_PER_POINT = 2 * 593408


def event_ms(fn, warmup=2, reps=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    times.sort()
    return times[len(times) // 2], times


def gyroid(n, dev, periods=4.0):
    """1.5 + gyroid(2 pi periods x) on [-1, 1]^3: a dense, non-trivial surface at iso 1.5."""
    xs = mesh.grid_axes((-1, -1, -1), (1, 1, 1), n, dev)
    w = torch.pi * periods
    x, y, z = (t * w for t in xs)
    sx, cx, sy, cy, sz, cz = torch.sin(x), torch.cos(x), torch.sin(y), torch.cos(y), torch.sin(z), torch.cos(z)
    return (1.5 + sx[:, None, None] * cy[None, :, None] + sy[None, :, None] * cz[None, None, :]
            + sz[None, None, :] * cx[:, None, None]).contiguous()


def mc_row(n, dev):
    g = gyroid(n, dev)
    iso, lo, hi = 1.5, (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)
    verts, faces, _ = mesh.marching_cubes(g, iso, lo, hi)
    V, F, N = verts.shape[0], faces.shape[0], n ** 3
    del verts, faces
    # kernel passes on preallocated buffers (the API call below adds allocation and the one read-back)
    G = _lib.load().mvip_mcubes_groups(n, n, n)
    tab = mesh.device_table(dev)
    flags = torch.empty(N, device=dev, dtype=torch.int16)
    wg = torch.empty((G, 2), device=dev, dtype=torch.int64)
    totals = torch.empty(3, device=dev, dtype=torch.int64)
    vid = torch.empty(N, device=dev, dtype=torch.int32)
    vb, nb = torch.empty((V, 3), device=dev), torch.empty((V, 3), device=dev)
    fb = torch.empty((F, 3), device=dev, dtype=torch.int32)

    def count():
        call('mvip_mcubes_count', ptr(g), n, n, n, iso, ptr(tab, torch.int8), ptr(flags, torch.int16), ptr(wg, torch.int64),
             ptr(totals, torch.int64), stream())

    def emit():
        call('mvip_mcubes_emit', ptr(g), n, n, n, iso, *lo, *hi, ptr(tab, torch.int8), ptr(flags, torch.int16),
             ptr(wg, torch.int64), V, F, ptr(vid, torch.int32), ptr(vb), ptr(nb), ptr(fb, torch.int32), stream())

    def both():
        count()
        emit()

    count()
    assert [int(x) for x in totals.cpu()] == [V, F, 0]
    t_count, _ = event_ms(count)
    t_emit, _ = event_ms(emit)
    t_passes, reps = event_ms(both)
    t_api, _ = event_ms(lambda: mesh.marching_cubes(g, iso, lo, hi))
    nbytes = 14 * N + 24 * V + 12 * F
    return {'grid': [n, n, n], 'field': 'gyroid, 4 periods, iso 1.5', 'grid_MB': round(4 * N / 1e6, 1),
            'vertices': V, 'triangles': F, 'ms_count_passes': round(t_count, 4), 'ms_emit_passes': round(t_emit, 4),
            'ms_all_passes': round(t_passes, 4), 'ms_all_passes_reps': [round(t, 4) for t in reps],
            'ms_api_call': round(t_api, 4), 'compulsory_bytes': nbytes,
            'TB_per_s_all_passes': round(nbytes / (t_passes * 1e-3) / 1e12, 3),
            'fraction_of_6.3_TB_s': round(nbytes / (t_passes * 1e-3) / HBM_BYTES_PER_S, 3),
            'note': 'grid exceeds the 256 MiB Infinity Cache: an HBM figure' if 4 * N > 256 * 2 ** 20
            else 'grid fits the 256 MiB Infinity Cache: not an HBM figure'}


def query_rows(n, dev):
    from oracle.weights import seeded_state_dict
    rows = []
    _, kw, _, _, _ = run.create_nerf(model_args(64), device=dev)
    kw['network_fine'].load_state_dict({k: torch.from_numpy(v) for k, v in seeded_state_dict(1).items()})
    for prec, name in ((0, 'fp32'), (1, 'split')):
        kw['network_fine'].inference_precision = prec
        t, reps = event_ms(lambda: mesh.density_grid(kw, (-1, -1, -1), (1, 1, 1), n), warmup=1, reps=3)
        rows.append({'model': 'mlp 8x256', 'precision': name, 'grid': [n, n, n], 'ms': round(t, 2),
                     'ms_reps': [round(x, 2) for x in reps], 'Mpoints_per_s': round(n ** 3 / t / 1e3, 1),
                     'TFLOP_per_s': round(n ** 3 * MLP_FLOP_PER_POINT / (t * 1e-3) / 1e12, 1)})
    del kw
    torch.manual_seed(0)
    _, kw, _, _, _ = run.create_nerf_tcnn(model_args(64), device=dev)
    t, reps = event_ms(lambda: mesh.density_grid(kw, (-1, -1, -1), (1, 1, 1), n), warmup=1, reps=3)
    rows.append({'model': 'hash grid (NeRF_TCNN)', 'precision': 'fp32 (the only one)', 'grid': [n, n, n], 'ms': round(t, 2),
                 'ms_reps': [round(x, 2) for x in reps], 'Mpoints_per_s': round(n ** 3 / t / 1e3, 1)})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profile_out', 'mesh_extract.json'))
    ap.add_argument('--commit', default='')
    a = ap.parse_args()
    dev = torch.device('cuda', 0)
    out = {'commit': a.commit, 'device': torch.cuda.get_device_name(0),
           'marching_cubes': [mc_row(256, dev), mc_row(512, dev)],
           'density_query': query_rows(256, dev)}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))
    return 0


if __name__ == '__main__':
    sys.exit(main())
