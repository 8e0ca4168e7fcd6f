"""Timing of TSDF depth-map fusion and of marching cubes on observed cells (profiles/tsdf_fusion.json), and
the two meshes of the scene-1 field (profiles/tsdf_scene1.json).

  python tools/tsdf_bench.py [--out profile_out/tsdf_fusion.json] [--commit SHA]
  python tools/tsdf_bench.py --scene1 [--iters 1500] [--out profile_out/tsdf_scene1.json] [--commit SHA]
  python tools/tsdf_bench.py --once            # one warm-up and one fusion: the run to put under a kernel trace

Default: 30 views of 378 x 504 (the benchmark's frame and focal length) of an analytic scene -- a wall and a box face in front
of it, the geometry of tests/warp_numpy.py -- seen by cameras on a shallow arc, fused onto a 256^3 lattice; milliseconds of one
ops.tsdf_fuse between device events (the median of windows of --reps calls after a warm-up), the bytes the fusion moves from
HBM computed from the shapes (hbm_bytes) and the share of the HBM peak that makes of the time; then the classification pass of
marching cubes on the fused lattice without and with the validity lattice (mvip_mcubes_count / mvip_mcubes_count_valid,
alternating in one loop), and the whole mesh.marching_cubes both ways.  The sigma-lattice query the fusion stands beside is
quoted from profiles/components.json, not measured again.

--scene1: the field of the 1,500-iteration recipe (tools/render_occupancy_ab.py::train_scene1) meshed both ways at 256^3 in
tools/extract_mesh.py's default box and in the cameras' frustum box: sigma = 10 (mesh.extract_mesh's way) and the TSDF of the
30 rendered views; for each the components of the inside lattice points, vertices and triangles, before and after largest=1,
and for the TSDF the observed share of the lattice.
"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12                    # bytes / s, specification
COPY_RATE = 6.29e12                  # float4 copy, bytes / s, measured
H, W, FOCAL = 378, 504, 383.65
WALL_Z, BOX_Z, BOX_X, BOX_Y = -4.0, -2.5, (-.4, .5), (-.3, .4)
BOX_MIN, BOX_MAX = (-1.6, -1.2, -4.4), (1.6, 1.2, -1.2)


def hbm_bytes(V, h, w, n_points, masked=False):
    """Bytes of one fusion from the shapes: 8 written per lattice point (tsdf, count); each view's disparity (and mask byte)
    fetched once -- the lattice's gathers revisit them through L2 and the Infinity Cache (one 378 x 504 view is 0.76 MB)."""
    return n_points * 8 + V * h * w * (5 if masked else 4)


def rot(ax, ay, az):
    cx, sx, cy, sy, cz, sz = math.cos(ax), math.sin(ax), math.cos(ay), math.sin(ay), math.cos(az), math.sin(az)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def analytic_views(V):
    """(disp [V, H, W] fp32, poses [V, 3, 4] fp32): cameras on an arc of +-0.9 about the scene's axis, turned toward it."""
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    dirs = np.stack([(x - W * .5) / FOCAL, -(y - H * .5) / FOCAL, -np.ones_like(x)], -1)
    disp, poses = [], []
    for v in range(V):
        s = -0.9 + 1.8 * v / max(V - 1, 1)
        o = np.array([s + 0.013, 0.21 * math.sin(2.3 * s) + 0.017, 0.05 * math.cos(1.7 * s) + 0.011])
        R = rot(0.02 * math.cos(3.1 * s) + 0.011, 0.25 * s + 0.007, 0.015 * math.sin(1.3 * s) + 0.009)
        d = dirs @ R.T
        t_wall, t_box = (WALL_Z - o[2]) / d[..., 2], (BOX_Z - o[2]) / d[..., 2]
        pb = o + t_box[..., None] * d
        hit = (t_box > 0) & (pb[..., 0] >= BOX_X[0]) & (pb[..., 0] <= BOX_X[1]) & (pb[..., 1] >= BOX_Y[0]) & (pb[..., 1] <= BOX_Y[1])
        disp.append(1.0 / np.where(hit, t_box, t_wall))
        poses.append(np.concatenate([R, o[:, None]], 1))
    return np.stack(disp).astype(np.float32), np.stack(poses).astype(np.float32)


def window_ms(fn, reps, windows=5):
    """Median over `windows` of (milliseconds of `reps` back-to-back calls between two device events) / reps, after one warm-up."""
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(windows):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / reps)
    return float(np.median(out)), [round(x, 4) for x in out]


def kernel_part(a, dev):
    from mvip_nerf_amd import _lib, mesh, ops
    from mvip_nerf_amd._lib import call, ptr, stream
    disp, poses = analytic_views(a.views)
    d, p = torch.from_numpy(disp).to(dev), torch.from_numpy(poses).to(dev)
    n = a.resolution
    step = max((BOX_MAX[k] - BOX_MIN[k]) / (n - 1) for k in range(3))
    trunc = 4.0 * step
    fuse = lambda: ops.tsdf_fuse(d, p, FOCAL, BOX_MIN, BOX_MAX, n, trunc)
    if a.once:
        fuse()
        t, c = fuse()
        torch.cuda.synchronize()
        return {'views': a.views, 'frame': [H, W], 'lattice': [n] * 3, 'observed_share': float((c > 0).float().mean())}
    ms, wins = window_ms(fuse, a.reps)
    t, c = fuse()
    nbytes = hbm_bytes(a.views, H, W, n ** 3)
    out = {'fusion': {'views': a.views, 'frame': [H, W], 'focal': FOCAL, 'lattice': [n] * 3, 'box_min': BOX_MIN, 'box_max': BOX_MAX, 'trunc': trunc,
                      'scene': 'analytic wall z = -4 and box face z = -2.5, cameras on an arc of +-0.9',
                      'ms': ms, 'ms_windows': wins, 'calls_per_window': a.reps, 'projections': a.views * n ** 3,
                      'projections_per_s': a.views * n ** 3 / (ms * 1e-3), 'bytes_from_shapes': nbytes, 'rate_bytes_per_s': nbytes / (ms * 1e-3),
                      'share_of_hbm_peak': nbytes / (ms * 1e-3) / HBM_PEAK, 'share_of_copy_rate': nbytes / (ms * 1e-3) / COPY_RATE,
                      'hbm_peak_bytes_per_s': HBM_PEAK, 'copy_rate_bytes_per_s': COPY_RATE,
                      'observed_share': float((c > 0).float().mean()), 'inside_share': float(((c > 0) & (t <= 0)).float().mean()),
                      'seen_by_all_share': float((c == a.views).float().mean())}}
    # the classification pass on the fused lattice, without and with the validity lattice, alternating
    valid = (c > 0).contiguous()
    g = torch.where(valid, 1.0 - t, torch.zeros((), device=dev)).contiguous()
    table = mesh.device_table(dev)
    G = _lib.load().mvip_mcubes_groups(n, n, n)
    flags = torch.empty(n ** 3, device=dev, dtype=torch.int16)
    wg = torch.empty((G, 2), device=dev, dtype=torch.int64)
    totals = torch.empty(3, device=dev, dtype=torch.int64)
    plain = lambda: call('mvip_mcubes_count', ptr(g), n, n, n, 1.0, ptr(table, torch.int8), ptr(flags, torch.int16), ptr(wg, torch.int64),
                         ptr(totals, torch.int64), stream())
    masked = lambda: call('mvip_mcubes_count_valid', ptr(g), ptr(valid, torch.bool), n, n, n, 1.0, ptr(table, torch.int8),
                          ptr(flags, torch.int16), ptr(wg, torch.int64), ptr(totals, torch.int64), stream())
    rows = {'plain': [], 'masked': []}
    for _ in range(5):
        for name, fn in (('plain', plain), ('masked', masked)):
            rows[name].append(window_ms(fn, a.count_reps, windows=1)[0])
    plain()
    tp = [int(x) for x in totals.cpu()]
    masked()
    tm = [int(x) for x in totals.cpu()]
    mp, mm = float(np.median(rows['plain'])), float(np.median(rows['masked']))
    whole = {name: window_ms(lambda v=v: mesh.marching_cubes(g, 1.0, BOX_MIN, BOX_MAX, valid=v), 5)[0] for name, v in (('plain', None), ('masked', valid))}
    out['classification'] = {'lattice': [n] * 3, 'ms_count': mp, 'ms_count_valid': mm, 'ms_windows_count': [round(x, 4) for x in rows['plain']],
                             'ms_windows_count_valid': [round(x, 4) for x in rows['masked']], 'overhead_ms': mm - mp, 'overhead_ratio': mm / mp,
                             'vertices_triangles_plain': tp[:2], 'vertices_triangles_masked': tm[:2],
                             'ms_marching_cubes_whole_plain': whole['plain'], 'ms_marching_cubes_whole_masked': whole['masked']}
    try:
        y = json.load(open(os.path.join(ROOT, 'profiles', 'components.json')))['yardstick']['ms_sigma_query_256_fp32']
        out['yardstick'] = {'ms_sigma_query_256_fp32_from_profiles_components_json': y, 'fusion_ms_over_sigma_query_ms': ms / y}
    except (OSError, KeyError):
        out['yardstick'] = 'profiles/components.json not found'
    return out


def scene1(a, dev):
    from mvip_nerf_amd import mesh, ops, prepare
    from tools import render_occupancy_ab as T
    scene = T.train_scene1(dev, a.iters)
    te, hwf, poses, near, far = scene['te'], (scene['H'], scene['W'], scene['focal']), scene['poses'], scene['near'], scene['far']
    poses = poses[:, :3, :4].contiguous().float()
    disp = prepare.render_disparities(te, hwf, poses, near, far)
    res = a.resolution
    out = {'fixture': 'tests/golden/scene1_small.npz', 'iterations': a.iters, 'views': int(poses.shape[0]), 'frame': [hwf[0], hwf[1]],
           'resolution': res, 'non_finite_rendered_pixels': int((~torch.isfinite(disp)).sum()), 'boxes': []}

    def describe(g, thr, lo, hi, valid=None):
        sizes = ops.grid_components(ops.grid_pack(g, thr), g.shape)[1]
        v, f, _ = mesh.marching_cubes(g, thr, lo, hi, valid=valid)
        rec = {'inside_points': int(sizes.sum()), 'components': int(sizes.shape[0]), 'largest_component_points': int(sizes.max()) if sizes.shape[0] else 0,
               'components_of_one_point': int((sizes == 1).sum()), 'vertices': int(v.shape[0]), 'triangles': int(f.shape[0])}
        if sizes.shape[0]:
            g1 = mesh.remove_floaters(g, thr, largest=1)
            v, f, _ = mesh.marching_cubes(g1, thr, lo, hi, valid=valid)
            rec.update(components_keep_largest_1=int(ops.grid_components(ops.grid_pack(g1, thr), g1.shape)[1].shape[0]),
                       vertices_keep_largest_1=int(v.shape[0]), triangles_keep_largest_1=int(f.shape[0]))
        return rec

    for name, (lo, hi) in (('tools/extract_mesh.py default box', ((-1.0,) * 3, (1.0,) * 3)), ('frustum box', T.scene_bounds(scene))):
        lo, hi = [float(v) for v in lo], [float(v) for v in hi]
        rec = {'box': name, 'box_min': lo, 'box_max': hi}
        grid = mesh.density_grid(te, lo, hi, res)
        rec['sigma_10'] = describe(grid, 10.0, lo, hi)
        del grid
        trunc = 4.0 * max((hi[k] - lo[k]) / (res - 1) for k in range(3))
        t, c = ops.tsdf_fuse(disp, poses, hwf[2], lo, hi, res, trunc)
        valid = c > 0
        g = torch.where(valid, 1.0 - t, torch.zeros((), device=dev))
        rec['tsdf'] = dict(describe(g, 1.0, lo, hi, valid=valid), trunc=trunc, observed_share=float(valid.float().mean()),
                           seen_by_all_share=float((c == poses.shape[0]).float().mean()))
        v, f, _ = mesh.marching_cubes(g, 1.0, lo, hi)
        rec['tsdf']['triangles_without_validity'] = int(f.shape[0])
        out['boxes'].append(rec)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--views', type=int, default=30)
    ap.add_argument('--resolution', type=int, default=256)
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--count-reps', type=int, default=200, help='calls per window of the classification pass')
    ap.add_argument('--once', action='store_true')
    ap.add_argument('--scene1', action='store_true')
    ap.add_argument('--iters', type=int, default=1500, help='training iterations of --scene1')
    ap.add_argument('--out', default=None)
    ap.add_argument('--commit', default='')
    a = ap.parse_args(argv)
    dev = torch.device('cuda', 0)
    out = scene1(a, dev) if a.scene1 else kernel_part(a, dev)
    if a.once:
        print(json.dumps(out))
        return 0
    out = dict(out, commit=a.commit, device=torch.cuda.get_device_name(0))
    path = a.out or os.path.join(ROOT, 'profile_out', 'tsdf_scene1.json' if a.scene1 else 'tsdf_fusion.json')
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, 'w') as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out, indent=1))
    return 0


if __name__ == '__main__':
    sys.exit(main())
