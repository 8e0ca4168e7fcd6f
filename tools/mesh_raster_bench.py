"""Mesh rasteriser timings (profiles/mesh_raster.json): csrc/raster.hip on the marching-cubes mesh of the analytic sphere
(radius 0.6) at 256^3, of the 4-period gyroid at 256^3 (2.5 M triangles, the size of the scene-1 sigma = 10 surface) and of the
gyroid's simplification by clustering at 8 lattice steps (larger triangles: the wave-cooperative path), each into 30 views of
378 x 504 on an orbit of radius 3 around the box.  HIP-event times, the median of 5 windows after a warm-up, on preallocated
buffers: the fragments entry point (its clear of the keys and the fragment launch), the clear alone (the same entry point with
no faces), the resolve launch without and with colours, and ops.mesh_rasterize as a whole (allocations and the flag read-back
included).  From the counting variant of the fragment kernel: the fragments that passed every test and the atomics actually
sent after the early-out load, and from those the implied rate of 8-byte atomics.  A record, not a gate.

Per fragment the kernel reads 8 bytes (the stored key) and sends at most one 8-byte atomic; per (face, view) it reads 12 bytes
of indices and 36 of positions (cached: a vertex is shared by about six faces) and does the fp64 projection of three vertices.

  python tools/mesh_raster_bench.py [--out profile_out/mesh_raster.json] [--size 256] [--views 30] [--commit HASH]
"""
import argparse
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from mvip_nerf_amd import mesh, ops                                  # noqa: E402
from mvip_nerf_amd._lib import ptr, stream, call                     # noqa: E402
from tools.mesh_bench import event_ms, gyroid                        # noqa: E402
from tools.mesh_ops_bench import sphere, LO, HI                      # noqa: E402

I32, I64, U8 = torch.int32, torch.int64, torch.uint8
H, W, FOCAL, NEAR = 378, 504, 400.0, 1e-3


def orbit(n, dev, radius=3.0):
    """n camera-to-world poses [n, 3, 4] on a tilted circle of `radius` around the origin, looking at it (down -z, y up)."""
    out = []
    for k in range(n):
        a = 2.0 * math.pi * k / n
        o = torch.tensor([radius * math.cos(a), 0.6 * math.sin(2 * a), radius * math.sin(a)], dtype=torch.float64)
        z = o / o.norm()
        x = torch.linalg.cross(torch.tensor([0.0, 1.0, 0.0], dtype=torch.float64), z)
        x = x / x.norm()
        y = torch.linalg.cross(z, x)
        out.append(torch.stack([x, y, z, o], 1))
    return torch.stack(out).to(device=dev, dtype=torch.float32).contiguous()


def row(name, v, f, poses):
    dev = v.device
    Nv, F, V = int(v.shape[0]), int(f.shape[0]), int(poses.shape[0])
    col = torch.randint(0, 256, (Nv, 3), device=dev, dtype=U8, generator=torch.Generator(device=dev).manual_seed(1))
    keys = torch.empty((V, H, W), device=dev, dtype=I64)
    flag = torch.empty(1, device=dev, dtype=I32)
    counts = torch.empty(2, device=dev, dtype=I64)
    disp = torch.empty((V, H, W), device=dev)
    face = torch.empty((V, H, W), device=dev, dtype=I32)
    rgb = torch.empty((V, H, W, 3), device=dev, dtype=U8)
    none = ptr(None)
    geom = (ptr(poses), V, H, W, FOCAL, NEAR)

    def fragments(n_faces=F, stats=none):
        call('mvip_raster_fragments', ptr(v), ptr(f, I32), Nv, n_faces, *geom, 0, ptr(keys, I64), ptr(flag, I32), stats, stream())

    def resolve(colours):
        call('mvip_raster_resolve', ptr(keys, I64), ptr(v), ptr(f, I32), ptr(col, U8) if colours else none, Nv, F, *geom, ptr(disp),
             ptr(face, I32), ptr(rgb, U8) if colours else none, stream())

    t_clear, _ = event_ms(lambda: fragments(0))
    t_frag, reps = event_ms(fragments)
    fragments(stats=ptr(counts, I64))
    n_frag, n_sent = (int(x) for x in counts.cpu())
    assert int(flag.cpu()) == 0
    t_res, _ = event_ms(lambda: resolve(False))
    t_res_rgb, _ = event_ms(lambda: resolve(True))
    t_api, _ = event_ms(lambda: ops.mesh_rasterize(v, f, poses, H, W, FOCAL, colors=col), warmup=1, reps=5)
    covered = int((face >= 0).sum())
    seen = int(torch.unique(face[face >= 0]).numel())
    launch = max(t_frag - t_clear, 1e-9)
    return {'mesh': name, 'vertices': Nv, 'triangles': F, 'views': V, 'image': [H, W], 'focal': FOCAL,
            'ms_fragments_entry_point': round(t_frag, 4), 'ms_fragments_entry_point_reps': [round(t, 4) for t in reps],
            'ms_clear_alone': round(t_clear, 4), 'ms_fragment_launch': round(t_frag - t_clear, 4),
            'ms_resolve': round(t_res, 4), 'ms_resolve_with_colours': round(t_res_rgb, 4),
            'ms_api_mesh_rasterize_with_colours': round(t_api, 4),
            'fragments': n_frag, 'atomics_sent': n_sent, 'share_of_fragments_sent': round(n_sent / max(n_frag, 1), 4),
            'fragments_per_face_and_view': round(n_frag / max(F * V, 1), 4),
            'atomic_bytes_per_second': round(8.0 * n_sent / (launch * 1e-3)),
            'face_views_per_second': round(F * V / (launch * 1e-3)),
            'covered_share_of_pixels': round(covered / (V * H * W), 4), 'triangles_that_win_a_pixel': seen,
            'share_of_triangles_that_win_a_pixel': round(seen / max(F, 1), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--views', type=int, default=30)
    ap.add_argument('--commit', default='')
    a = ap.parse_args()
    dev = torch.device('cuda', 0)
    a.out = a.out or os.path.join(ROOT, 'profile_out', 'mesh_raster.json')
    n = a.size
    poses = orbit(a.views, dev)
    rows = []
    v, f, _ = mesh.marching_cubes(sphere(n, dev), 1.0, LO, HI)
    rows.append(row('analytic sphere, radius 0.6, iso 1', v, f, poses))
    v, f, _ = mesh.marching_cubes(gyroid(n, dev), 1.5, LO, HI)
    rows.append(row('gyroid, 4 periods, iso 1.5', v, f, poses))
    cv, cf, _, _ = ops.mesh_cluster(v, f, None, None, 8 * 2.0 / (n - 1), 'quadric')
    rows.append(row('the gyroid clustered at 8 lattice steps', cv, cf, poses))
    out = {'commit': a.commit, 'device': torch.cuda.get_device_name(0), 'small_box_limit_pixels': 16, 'rows': rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out))
    return 0


if __name__ == '__main__':
    sys.exit(main())
