"""Occupancy-grid empty-space skipping (mvip_nerf_amd/occupancy.py, csrc/occupancy.hip) against the ordinary render, in
ONE process, the two variants alternated, device events around whole frames.

Trains the scene-1 fixture (tests/golden/scene1_small.npz, view 14 held out) with the recipe of
tests/test_configs.py::test_heldout_psnr_hip_vs_oracle_within_0p05_dB (1,500 iterations of 4,096 rays), builds grids over
mesh.frustum_bounds of the cameras for a sweep of thresholds, and per threshold records: the occupied fraction of the
grid, the kept fraction of samples per pass, ms per frame with and without the grid at the headline size (378 x 504, 64
coarse + 128 fine evaluations per ray), the PSNR between the two frames, and the change of PSNR against the ground truth
(at the fixture's own 141 x 252, where the ground truth exists).  Also: the grid build time split into the density query
and the build / dilate kernels, and two synthetic grids on the same field -- all bits set (pure overhead of compact +
scatter + the points entry point against the ray entry point) and a ball of radius 0.45 of the box at 50 % of its cells.
Prints one JSON and writes it to $MVIP_PROFILE_OUT/occupancy_ab.json (default folder: profile_out/).

  python tools/render_occupancy_ab.py [--iters 1500] [--repeats 3]
"""
import argparse
import json
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from mvip_nerf_amd import mesh, ops, run                                      # noqa: E402
from mvip_nerf_amd.occupancy import OccupancyGrid, DEFAULT_THRESHOLD           # noqa: E402

FIXTURE = os.path.join(ROOT, 'tests', 'golden', 'scene1_small.npz')
HELD = 14
THRESHOLDS = (0.0, 0.01, 0.1, 0.5, 1.0, 2.0, 5.0, 10.0)
HEADLINE = (378, 504)
CELLS, SAMPLES_PER_CELL, DILATE = 128, 2, 1                                    # from_model's defaults


def train_args():
    return types.SimpleNamespace(
        multires=10, i_embed=0, use_viewdirs=True, multires_views=4, N_importance=64, alpha_model_path=None, netdepth=8,
        netwidth=256, netdepth_fine=8, netwidth_fine=256, netchunk=65536, lrate=5e-4, basedir='/tmp/mvip_occ', expname='none',
        ft_path=None, no_reload=True, perturb=1., N_samples=64, white_bkgd=False, raw_noise_std=1., dataset_type='llff',
        no_ndc=True, lindisp=False, sigma_loss=False)


def train_scene1(device, iters=1500, precision=0):
    """The 1,500-iteration photometric recipe of tests/test_configs.py on the scene-1 fixture.  Returns a dict: `te` (the
    test-time render kwargs with near / far), images, poses, H, W, focal, near, far, held (the held-out view)."""
    from mvip_nerf_amd.run_nerf_helpers import img2mse
    d = np.load(FIXTURE)
    images = torch.from_numpy(d['images'].astype(np.float32) / 255.).to(device)
    poses = torch.from_numpy(d['poses'][:, :, :4]).to(device)
    Nv, H, W, _ = images.shape
    focal = float(d['poses'][0, 2, 4]) * (H / float(d['poses'][0, 0, 4]))
    near, far = float(d['bds'].min() * .9), float(d['bds'].max() * 1.)
    i_train = [i for i in range(Nv) if i != HELD]
    torch.manual_seed(0)
    tr, te, _, grad_vars, opt = run.create_nerf(train_args(), device=device)
    for net in (tr['network_fn'], tr['network_fine']):
        net.train_precision = net.inference_precision = precision
    kw_tr = {k: v for k, v in tr.items() if k not in ('ndc', 'use_viewdirs')}
    g = torch.Generator(device=device).manual_seed(0)
    for it in range(iters):
        v = i_train[int(torch.randint(0, len(i_train), (1,), generator=g, device=device))]
        sel = torch.randint(0, H * W, (4096,), generator=g, device=device)
        rows = ops.ray_rows_from_pose(poses[v], H, W, focal, near, far, sel=sel)
        r = run.batchify_rays(rows, 1 << 15, **kw_tr)
        tgt = images[v].reshape(-1, 3)[sel]
        loss = img2mse(r['rgb_map'], tgt) + img2mse(r['rgb0'], tgt)
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
    return dict(te=dict(te, near=near, far=far), images=images, poses=poses, H=H, W=W, focal=focal, near=near, far=far,
                held=HELD)


def scene_bounds(scene):
    """The default box: every camera's frustum between near and far."""
    return mesh.frustum_bounds(scene['poses'], (scene['H'], scene['W'], scene['focal']), scene['near'], scene['far'])


def render_view(scene, H, W, focal, occupancy=None):
    """[rgb, disp, acc, depth, extras] of the held-out pose, no grad."""
    with torch.no_grad():
        return run.render(H, W, focal, chunk=1 << 15, c2w=scene['poses'][scene['held']], occupancy=occupancy, **scene['te'])


def psnr(a, b):
    """dB; None for identical frames."""
    mse = float(((a - b) ** 2).mean())
    return None if mse == 0.0 else -10.0 * float(np.log10(mse))


def kept_fractions(grid):
    s = grid.stats
    return {'coarse': s['kept_coarse'] / max(1, s['samples_coarse']), 'fine': s['kept_fine'] / max(1, s['samples_fine'])}


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def ball_grid(bmin, bmax, cells, device, radius=0.45):
    """Cells whose centre lies within `radius` (in units of the box extent per axis) of the box centre."""
    ax = [(torch.arange(c, dtype=torch.float32) + 0.5) / c - 0.5 for c in cells]
    X, Y, Z = torch.meshgrid(*ax, indexing='ij')
    occ = (X * X + Y * Y + Z * Z <= radius * radius).reshape(-1).numpy()
    bits = np.zeros(ops.occupancy_words(cells) * 32, np.uint8)
    bits[:occ.size] = occ
    words = np.packbits(bits.reshape(-1, 32), axis=1, bitorder='little').reshape(-1).view('<u4').view(np.int32)
    return OccupancyGrid(bmin, bmax, cells, torch.from_numpy(words.copy()).to(device))


def ab_frames(scene, grid, repeats):
    """ms per headline-size frame, ordinary / grid alternated (both warmed first), and the kept fractions of one frame."""
    H, W = HEADLINE
    focal = scene['focal'] * W / scene['W']
    render_view(scene, H, W, focal)
    render_view(scene, H, W, focal, grid)
    plain, skipped = [], []
    for _ in range(repeats):
        plain.append(event_ms(lambda: render_view(scene, H, W, focal)))
        grid.reset_stats()
        skipped.append(event_ms(lambda: render_view(scene, H, W, focal, grid)))
    return plain, skipped, kept_fractions(grid)


def overhead_only(dev, repeats):
    """The full grid's cost on the bench frame: every sample is kept, so the difference to the ordinary frame is the compact
    / scatter passes, the read-back of K and the points entry point against the ray entry point."""
    import bench
    torch.manual_seed(0)
    _, te, *_ = run.create_nerf(bench.make_args(), device=dev)
    scene = dict(te=dict(te, near=bench.NEAR, far=bench.FAR), poses=bench.orbit_pose(0, dev)[None], held=0, W=bench.W,
                 focal=bench.FOCAL)
    cells = (CELLS,) * 3
    full = OccupancyGrid((-10, -10, -10), (10, 10, 10), cells,
                         torch.full((ops.occupancy_words(cells),), -1, dtype=torch.int32, device=dev))
    plain, skipped, kept = ab_frames(scene, full, repeats)
    out = {'what': 'all-bits-set grid on the bench frame, random-weight model', 'kept_fraction': kept, 'ms_ordinary': plain,
           'ms_grid': skipped}
    print(json.dumps(out, indent=1))
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--iters', type=int, default=1500)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--overhead-only', action='store_true',
                    help='no training: frames of a random-weight model with and without the all-bits-set grid (for a kernel trace)')
    a = ap.parse_args(argv)
    dev = torch.device('cuda', 0)
    if a.overhead_only:
        return overhead_only(dev, a.repeats)
    scene = train_scene1(dev, a.iters)
    te, H, W, focal = scene['te'], scene['H'], scene['W'], scene['focal']
    bmin, bmax = scene_bounds(scene)
    gt = scene['images'][scene['held']]
    base = render_view(scene, H, W, focal)[0]
    out = {'scene': {'fixture': 'tests/golden/scene1_small.npz', 'iterations': a.iters, 'held_out_view': scene['held'],
                     'psnr_frame': [H, W], 'timed_frame': list(HEADLINE), 'samples': '64 coarse + 128 fine evaluations per ray',
                     'bound_min': [float(v) for v in bmin], 'bound_max': [float(v) for v in bmax]},
           'grid': {'cells': CELLS, 'samples_per_cell': SAMPLES_PER_CELL, 'dilate': DILATE, 'networks': ['coarse', 'fine']},
           'default_threshold': DEFAULT_THRESHOLD, 'psnr_vs_ground_truth_ordinary': psnr(base, gt), 'sweep': []}

    # grid build time: the density query of both networks, and the build + dilate kernels on its result
    n = CELLS * SAMPLES_PER_CELL + 1
    mesh.density_grid(te, bmin, bmax, n, network='fine')
    sig = {}
    q_ms = sum(event_ms(lambda w=w: sig.__setitem__(w, mesh.density_grid(te, bmin, bmax, n, network=w))) for w in ('coarse', 'fine'))
    OccupancyGrid.from_density(sig['fine'], bmin, bmax, 1.0, SAMPLES_PER_CELL, DILATE)
    k_ms = sum(event_ms(lambda w=w: OccupancyGrid.from_density(sig[w], bmin, bmax, 1.0, SAMPLES_PER_CELL, DILATE)) for w in ('coarse', 'fine'))
    out['grid_build_ms'] = {'density_query_two_networks': q_ms, 'build_and_dilate_kernels_two_networks': k_ms,
                            'points_per_network': n ** 3}
    out['sigma_quantiles_fine'] = {str(q): float(torch.quantile(sig['fine'].reshape(-1)[::97].float(), q)) for q in (0.5, 0.9, 0.99)}

    spread = []
    for thr in THRESHOLDS:
        grid = OccupancyGrid.from_model(te, bmin, bmax, cells=CELLS, threshold=thr, samples_per_cell=SAMPLES_PER_CELL, dilate=DILATE)
        grid.reset_stats()
        small = render_view(scene, H, W, focal, grid)[0]
        kept_small = kept_fractions(grid)
        plain, skipped, kept = ab_frames(scene, grid, a.repeats)
        spread += plain
        out['sweep'].append({
            'threshold': thr, 'occupied_fraction': grid.occupied_fraction(), 'kept_fraction_timed_frame': kept,
            'kept_fraction_psnr_frame': kept_small, 'ms_ordinary': plain, 'ms_grid': skipped,
            'psnr_grid_vs_ordinary': psnr(small, base), 'psnr_vs_ground_truth_grid': psnr(small, gt),
            'delta_psnr_vs_ground_truth': psnr(small, gt) - psnr(base, gt)})
    out['ordinary_ms_spread_max_minus_min'] = max(spread) - min(spread)
    out['ordinary_ms_mean'] = sum(spread) / len(spread)

    cells = (CELLS,) * 3
    full = OccupancyGrid(bmin, bmax, cells, torch.full((ops.occupancy_words(cells),), -1, dtype=torch.int32, device=dev))
    out['synthetic'] = {}
    for name, grid in (('full_grid', full), ('ball_0p45', ball_grid(bmin, bmax, cells, dev))):
        plain, skipped, kept = ab_frames(scene, grid, a.repeats)
        out['synthetic'][name] = {'occupied_fraction': grid.occupied_fraction(), 'kept_fraction': kept, 'ms_ordinary': plain,
                                  'ms_grid': skipped}
    print(json.dumps(out, indent=1))
    out_dir = os.environ.get('MVIP_PROFILE_OUT', 'profile_out')
    os.makedirs(out_dir, exist_ok=True)
    json.dump(out, open(os.path.join(out_dir, 'occupancy_ab.json'), 'w'), indent=1)


if __name__ == '__main__':
    main()
