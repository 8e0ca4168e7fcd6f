"""How far the meshes of a field lie from what its renderer sees: the sigma mesh (mesh.extract_mesh) and the TSDF mesh
(mesh.fuse_depths of the rendered disparities) of one model, each as extracted and after --smooth / --simplify, rasterised back
into the cameras (mesh.render_views, csrc/raster.hip) and compared with prepare.render_disparities of the same cameras.  Prints
per stage: triangles, the triangles that win a pixel in at least one view (mesh.visible_faces), the share of the pixels the
mesh covers, and the depth L1 / L2 of its disparity against the rendered one over the covered pixels
(evaluate.mesh_depth_metrics).

  python tools/mesh_fidelity.py --fixture [--iters 1500] [--out report.json] ...
  python tools/mesh_fidelity.py CKPT.tar --datadir SCENE [--factor 4] ...
  python tools/mesh_fidelity.py --seeded ...
      [--resolution 256] [--threshold 10] [--bound-min x y z --bound-max x y z] [--view-step S]
      [--smooth ITERS] [--simplify STEPS] [--simplify-placement quadric|mean]

--fixture trains the scene-1 fixture, a checkpoint comes with --datadir / --factor (the cameras are taken the way
tools/extract_mesh.py --tsdf takes them).  --seeded needs neither: the seeded 8 x 256 pair of the tests with its density head
rescaled to sigma' = 4 (sigma - median) / std over one camera's sample points, ten orbit cameras of 45 x 60, and by default the
90th percentile of its lattice as the threshold -- a model that renders something, not a trained scene.  Without
--bound-min / --bound-max the box is the cameras' frustum box (mesh.frustum_bounds).
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from mvip_nerf_amd import evaluate, mesh, ops, prepare, run          # noqa: E402


def seeded_scene(dev):
    import bench
    from oracle.weights import seeded_state_dict
    _, te, _, _, _ = run.create_nerf(bench.make_args(), device=dev)
    sel = torch.from_numpy(np.random.RandomState(99).randint(0, bench.H * bench.W, 2000)).to(dev)
    rows = ops.ray_rows_from_pose(bench.orbit_pose(0, dev), bench.H, bench.W, bench.FOCAL, bench.NEAR, bench.FAR, sel=sel)
    z = ops.stratified_z(rows, 64, True)
    pts = (rows[:, None, 0:3] + rows[:, None, 3:6] * z[:, :, None]).reshape(-1, 3)
    dirs = rows[:, None, 8:11].expand(-1, 64, -1).reshape(-1, 3).contiguous()
    for net, seed in ((te['network_fn'], 1), (te['network_fine'], 2)):
        net.load_state_dict({k: torch.from_numpy(w) for k, w in seeded_state_dict(seed).items()})
        with torch.no_grad():
            sigma = net.query_points(pts, dirs)[:, 3]
            scale = 4.0 / float(sigma.std())
            net.alpha_linear.bias.copy_((net.alpha_linear.bias - sigma.median()) * scale)
            net.alpha_linear.weight.mul_(scale)
        net.invalidate_packed()
    h, w = 45, 60
    poses = torch.stack([bench.orbit_pose(k, dev)[:3, :4] for k in range(0, 60, 6)]).contiguous()
    return te, (h, w, bench.FOCAL * w / bench.W), poses, bench.NEAR, bench.FAR, {'model': 'seeded 8 x 256 pair, rescaled density head'}


def stage(name, m, hwf, poses, disp):
    seen = int(mesh.visible_faces(m, hwf, poses).sum()) if m.faces.shape[0] else 0
    rep = evaluate.mesh_depth_metrics(m, hwf, poses, disp)['mean']
    row = {'stage': name, 'triangles': int(m.faces.shape[0]), 'vertices': int(m.verts.shape[0]), 'visible_triangles': seen,
           'coverage': rep['coverage'], 'depth_l1': rep['depth_l1'], 'depth_l2': rep['depth_l2']}
    fmt = lambda x: 'none' if x is None else f'{x:.5f}'
    print(f'{name:<34} {row["triangles"]:>10,} triangles  {seen:>10,} visible ({seen / max(row["triangles"], 1):6.1%})  '
          f'coverage {fmt(row["coverage"])}  depth L1 {fmt(row["depth_l1"])}  L2 {fmt(row["depth_l2"])}')
    return row


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('ckpt', nargs='?')
    ap.add_argument('--fixture', action='store_true')
    ap.add_argument('--seeded', action='store_true')
    ap.add_argument('--iters', type=int, default=1500, help='training iterations of --fixture')
    ap.add_argument('--datadir')
    ap.add_argument('--factor', type=int, default=4)
    ap.add_argument('--resolution', type=int, default=256)
    ap.add_argument('--threshold', type=float, default=None, help='sigma level (default 10; --seeded: the 90th percentile)')
    ap.add_argument('--bound-min', type=float, nargs=3, default=None)
    ap.add_argument('--bound-max', type=float, nargs=3, default=None)
    ap.add_argument('--view-step', type=int, default=1, metavar='S', help='use every S-th view')
    ap.add_argument('--smooth', type=int, default=0, metavar='ITERS')
    ap.add_argument('--simplify', type=float, default=0.0, metavar='STEPS')
    ap.add_argument('--simplify-placement', choices=('quadric', 'mean'), default='quadric')
    ap.add_argument('--out', default=None, help='also write the rows as JSON')
    a = ap.parse_args(argv)
    if int(a.fixture) + int(a.seeded) + int(bool(a.ckpt)) != 1 or bool(a.ckpt) != bool(a.datadir):
        ap.error('one of --fixture, --seeded, or a checkpoint with --datadir')
    if (a.bound_min is None) != (a.bound_max is None) or a.view_step < 1 or a.smooth < 0 or not a.simplify >= 0:
        ap.error('--bound-min and --bound-max come together; --view-step >= 1; --smooth, --simplify >= 0')
    dev = torch.device('cuda', 0)
    if a.seeded:
        te, hwf, poses, near, far, source = seeded_scene(dev)
    else:
        from tools import propagate_masks as P
        te, hwf, poses, _, _, _, near, far, source = (P.fixture_scene(dev, a.iters) if a.fixture
                                                      else P.checkpoint_scene(dev, a.ckpt, a.datadir, a.factor))
    poses = torch.as_tensor(poses).to(dev)[::a.view_step, :3, :4].contiguous().float()
    lo, hi = (a.bound_min, a.bound_max) if a.bound_min is not None else mesh.frustum_bounds(poses, hwf, near, far)
    lo32, hi32 = mesh._bounds(lo, hi)
    h = max(float((hi32[k] - lo32[k]) / np.float32(a.resolution - 1)) for k in range(3))
    disp = prepare.render_disparities(te, hwf, poses, near, far)
    grid = mesh.density_grid(te, lo32, hi32, a.resolution)
    thr = a.threshold if a.threshold is not None else (float(np.percentile(grid.cpu().numpy(), 90)) if a.seeded else 10.0)
    print(f'{source}: {poses.shape[0]} views of {hwf[0]} x {hwf[1]}, lattice {a.resolution}^3 in {[round(float(v), 4) for v in lo32]} .. '
          f'{[round(float(v), 4) for v in hi32]}, sigma threshold {thr:.4g}')

    def cleaned(m):
        out = mesh.smooth(m, a.smooth) if a.smooth else m
        return mesh.simplify(out, a.simplify * h, a.simplify_placement) if a.simplify else out

    what = ' + '.join(([f'{a.smooth} Taubin'] if a.smooth else []) + ([f'clustered at {a.simplify:g} steps'] if a.simplify else []))
    rows = []
    v, f, n = mesh.marching_cubes(grid, thr, lo32, hi32)
    del grid
    for name, m in (('sigma mesh', mesh.Mesh(v, f, n, None)),
                    ('TSDF mesh', mesh.fuse_depths(disp, poses, float(hwf[2]), lo32, hi32, a.resolution))):
        rows.append(stage(name, m, hwf, poses, disp))
        if m.faces.shape[0]:
            seen = mesh.keep_faces(m, mesh.visible_faces(m, hwf, poses))
            rows.append(stage(f'{name}, unseen faces dropped', seen, hwf, poses, disp))
            if what:
                rows.append(stage(f'{name}, {what}', cleaned(m), hwf, poses, disp))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            json.dump({'source': source, 'views': int(poses.shape[0]), 'image': [int(hwf[0]), int(hwf[1])], 'resolution': a.resolution,
                       'bound_min': [float(x) for x in lo32], 'bound_max': [float(x) for x in hi32], 'threshold': thr,
                       'smooth': a.smooth, 'simplify': a.simplify, 'rows': rows}, fh, indent=1)
    return 0


if __name__ == '__main__':
    sys.exit(main())
