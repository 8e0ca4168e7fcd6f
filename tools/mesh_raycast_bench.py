"""Mesh ray casting timings (profiles/mesh_raycast.json; csrc/mesh_raycast.hip) on the marching-cubes mesh of the 4-period gyroid
of tools/mesh_ops_bench.py (256^3: 2.5 M triangles).

Camera rays: a 378 x 504 frame from outside the box and one from inside the surface (a fly-through, where the rasteriser drops
every face that reaches behind its near plane): HIP-event time of ops.mesh_cast_rays with a given grid (one launch and its
output allocations), rays per second, ray-face tests and cells per ray and the lane utilisation of the face loop (tests / (64 x
the busiest lane's tests, summed over the waves)) from the counting variant; the any-hit kernel on the same rays; next to it
ops.mesh_rasterize for the same view, the share of pixels where the two name the same face and the largest disparity difference
on those (they differ by the rasteriser's 8-bit sub-pixel snapping and its fill rule: a record, not a gate).
The openness sweep: ops.mesh_face_openness at K = 32 over every face, the rays it casts (the directions with N . d != 0), the same
counters, and how many faces mesh.drop_interior would keep.  The median of 5 windows after a warm-up.

--scene1: the sigma = 10 mesh of the scene-1 fixture field (trained here, --iters iterations): its triangles, those left by
keeping what a training camera sees (mesh.visible_faces) and those left by mesh.drop_interior at K = 32.

  python tools/mesh_raycast_bench.py [--size 256] [--scene1 [--iters 1500]] [--out-dir profile_out] [--commit HASH]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from mvip_nerf_amd import mesh, ops                                  # noqa: E402
from tools.mesh_bench import event_ms, gyroid                        # noqa: E402

LO, HI = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)
H, W, FOCAL, NEAR, FAR = 378, 504, 400.0, 0.05, 10.0
VIEWS = {'outside': [[1, 0, 0, 0.1], [0, 1, 0, -0.05], [0, 0, 1, 3.2]],
         'inside': [[1, 0, 0, 0.03], [0, 1, 0, 0.02], [0, 0, 1, 0.6]]}
K = 32


def counters(stats, rays):
    tests, slots, cells = (int(x) for x in stats.cpu())
    return {'ray_face_tests_per_ray': round(tests / max(rays, 1), 2), 'cells_per_ray': round(cells / max(rays, 1), 2),
            'lane_utilisation_of_the_face_loop': round(tests / max(slots, 1), 4)}


def camera_rays(v, f, g, dev):
    rows = []
    m = mesh.Mesh(v, f, None, None)
    for name, pose in VIEWS.items():
        pose = torch.tensor(pose, device=dev, dtype=torch.float32)
        ro, rd = ops.get_rays(H, W, FOCAL, pose)
        o, d = ro.reshape(-1, 3).contiguous(), rd.reshape(-1, 3).contiguous()
        N = int(o.shape[0])
        cast = lambda **kw: ops.mesh_cast_rays(o, d, v, f, tmin=NEAR, tmax=FAR, grid=g, **kw)
        t_c, reps = event_ms(cast)
        t_b, _ = event_ms(lambda: cast(return_bary=True))
        t_s, _ = event_ms(lambda: cast(return_stats=True))
        t_a, _ = event_ms(lambda: ops.mesh_occluded(o, d, v, f, tmin=NEAR, tmax=FAR, grid=g))
        face, depth, stats = cast(return_stats=True)
        occ, stats_any = ops.mesh_occluded(o, d, v, f, tmin=NEAR, tmax=FAR, grid=g, return_stats=True)
        assert bool((occ == (face >= 0)).all())
        t_r, _ = event_ms(lambda: ops.mesh_rasterize(v, f, pose[None], H, W, FOCAL, near=NEAR))
        rdisp, rface, _ = ops.mesh_rasterize(v, f, pose[None], H, W, FOCAL, near=NEAR)
        cdisp, cface, _ = mesh.cast_views(m, (H, W, FOCAL), pose[None], NEAR, FAR, colors=False)
        both = (cface == rface) & (cface >= 0)
        rows.append(dict({'view': name, 'rays': N, 'ms_cast': round(t_c, 4), 'ms_reps': [round(t, 4) for t in reps],
                          'ms_cast_with_bary': round(t_b, 4), 'ms_cast_counting_variant': round(t_s, 4), 'ms_any_hit': round(t_a, 4),
                          'rays_per_second': round(N / (t_c * 1e-3)), 'share_of_rays_that_hit': round(float((face >= 0).float().mean()), 4)},
                         **counters(stats, N),
                         **{'any_hit_' + k: x for k, x in counters(stats_any, N).items()},
                         **{'ms_mesh_rasterize': round(t_r, 4),
                            'pixels_covered_by_cast_and_by_raster': [int((cface >= 0).sum()), int((rface >= 0).sum())],
                            'share_of_pixels_with_the_same_face': round(float((cface == rface).float().mean()), 5),
                            'share_of_covered_pixels_with_the_same_face': round(float(both.sum()) / max(int(((cface >= 0) | (rface >= 0)).sum()), 1), 5),
                            'max_disparity_difference_on_those': float((cdisp - rdisp)[both].abs().max()) if bool(both.any()) else None}))
    return rows


def openness(v, f, g, dev):
    dirs = torch.from_numpy(mesh.fibonacci_directions(K)).to(dev)
    run = lambda **kw: ops.mesh_face_openness(v, f, dirs, grid=g, **kw)
    t_o, reps = event_ms(run, warmup=1, reps=5)
    fo, ft, bo, bt, stats = run(return_stats=True)
    rays = int(ft.sum()) + int(bt.sum())
    F = int(f.shape[0])
    return dict({'directions': K, 'faces': F, 'rays': rays, 'ms_face_openness': round(t_o, 3), 'ms_reps': [round(t, 3) for t in reps],
                 'rays_per_second': round(rays / (t_o * 1e-3)), 'share_of_rays_open': round((int(fo.sum()) + int(bo.sum())) / max(rays, 1), 5),
                 'faces_kept_two_sided': int((fo + bo > 0).sum()), 'faces_kept_front_only': int((fo > 0).sum())}, **counters(stats, rays))


def scene1(dev, iters, resolution):
    import numpy as np
    from tools import propagate_masks as P
    te, hwf, poses, _, _, _, near, far, source = P.fixture_scene(dev, iters)
    poses = torch.as_tensor(poses).to(dev)[:, :3, :4].contiguous().float()
    lo32, hi32 = mesh._bounds(*mesh.frustum_bounds(poses, hwf, near, far))
    v, f, n = mesh.marching_cubes(mesh.density_grid(te, lo32, hi32, resolution), 10.0, lo32, hi32)
    sigma = mesh.Mesh(v, f, n, None)
    seen = mesh.visible_faces(sigma, hwf, poses)
    fo, _, bo, _ = mesh.face_openness(sigma, K)
    return {'source': source, 'resolution': resolution, 'threshold': 10.0, 'views': int(poses.shape[0]), 'triangles': int(f.shape[0]),
            'triangles_after_drop_unseen': int(seen.sum()), 'triangles_after_drop_interior_32': int((fo + bo > 0).sum()),
            'triangles_after_drop_interior_32_front_only': int((fo > 0).sum()),
            'seen_but_dropped_as_interior': int((seen & ~(fo + bo > 0)).sum()), 'lattice_step': float(np.max((hi32 - lo32) / (resolution - 1)))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--scene1', action='store_true')
    ap.add_argument('--iters', type=int, default=1500, help='training iterations of --scene1')
    ap.add_argument('--out-dir', default=os.path.join(ROOT, 'profile_out'))
    ap.add_argument('--commit', default='')
    a = ap.parse_args()
    dev = torch.device('cuda', 0)
    v, f, _ = mesh.marching_cubes(gyroid(a.size, dev), 1.5, LO, HI)
    g = ops.mesh_face_grid(v, f)
    out = {'commit': a.commit, 'device': torch.cuda.get_device_name(0), 'mesh': f'gyroid, 4 periods, iso 1.5, {a.size}^3',
           'vertices': int(v.shape[0]), 'triangles': int(f.shape[0]), 'cells': list(g.cells), 'pairs': g.n_pairs,
           'frame': [H, W, FOCAL, NEAR, FAR], 'camera_rays': camera_rays(v, f, g, dev), 'openness_sweep': openness(v, f, g, dev)}
    if a.scene1:
        out['scene1_sigma_mesh'] = scene1(dev, a.iters, a.size)
    os.makedirs(a.out_dir, exist_ok=True)
    with open(os.path.join(a.out_dir, 'mesh_raycast.json'), 'w') as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out), flush=True)
    return 0


if __name__ == '__main__':
    sys.exit(main())
