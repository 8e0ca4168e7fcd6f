"""Ray distortion loss (mip-NeRF 360 eq. 15; csrc/distortion.hip, run.render_rays(distortion=True)) as a regulariser of the
photometric training loop, A/B over its weight, in ONE process with sequential runs.

Per lambda in {0, 0.001, 0.01, 0.1} (0.01 is the paper's value; nothing here is tuned): the scene-1 fixture
(tests/golden/scene1_small.npz, views 4, 14, 24 held out) is trained with the 1,500-iteration, 4,096-ray loop of
tools/train_real_scene.py from the same seeds, the loss being img2mse(rgb_map) + img2mse(rgb0) + lambda * mean(dist_loss +
dist_loss0).  Recorded per run: ms per iteration, held-out PSNR, the mean dist_loss of the held-out frames, and -- the fog the
occupancy write-up reports -- the occupied share of OccupancyGrid.from_model(cells=128, threshold=5.0, samples_per_cell=2,
dilate=1) over mesh.frustum_bounds, the kept coarse / fine sample shares of a frame rendered with that grid and that
frame's time against the ordinary frame's (device events, alternated, as tools/render_occupancy_ab.py does).
A record, not a gate.  Prints one JSON and writes it to $MVIP_PROFILE_OUT/distortion_ab.json (default folder: profile_out/).

  python tools/distortion_ab.py [--iters 1500] [--lambdas 0 0.001 0.01 0.1] [--repeats 3]
"""
import argparse
import json
import os
import sys
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from mvip_nerf_amd import mesh, ops, run                                      # noqa: E402
from mvip_nerf_amd.occupancy import OccupancyGrid                              # noqa: E402
from mvip_nerf_amd.run_nerf_helpers import img2mse, mse2psnr                   # noqa: E402

FIXTURE = os.path.join(ROOT, 'tests', 'golden', 'scene1_small.npz')
HELD = (4, 14, 24)
LAMBDAS = (0.0, 0.001, 0.01, 0.1)
HEADLINE = (378, 504)
GRID = dict(cells=128, threshold=5.0, samples_per_cell=2, dilate=1)


def train_args():
    return types.SimpleNamespace(
        multires=10, i_embed=0, use_viewdirs=True, multires_views=4, N_importance=64, alpha_model_path=None, netdepth=8,
        netwidth=256, netdepth_fine=8, netwidth_fine=256, netchunk=65536, lrate=5e-4, basedir='/tmp/mvip_dist', expname='none',
        ft_path=None, no_reload=True, perturb=1., N_samples=64, white_bkgd=False, raw_noise_std=1., dataset_type='llff',
        no_ndc=True, lindisp=False, sigma_loss=False)


def load_scene(device):
    d = np.load(FIXTURE)
    images = torch.from_numpy(d['images'].astype(np.float32) / 255.).to(device)
    poses = torch.from_numpy(d['poses'][:, :, :4]).to(device)
    Nv, H, W, _ = images.shape
    focal = float(d['poses'][0, 2, 4]) * (H / float(d['poses'][0, 0, 4]))
    return dict(images=images, poses=poses, H=H, W=W, focal=focal, near=float(d['bds'].min() * .9), far=float(d['bds'].max() * 1.),
                train=[i for i in range(Nv) if i not in HELD])


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def train(scene, lam, iters, device):
    """The loop of tools/train_real_scene.py with the distortion term; returns (test kwargs, ms per iteration, loss log)."""
    torch.manual_seed(0)
    args = train_args()
    tr, te, _, _, opt = run.create_nerf(args, device=device)
    kw = {k: v for k, v in tr.items() if k not in ('ndc', 'use_viewdirs')}
    if lam > 0:
        kw['distortion'] = True
    g = torch.Generator(device=device).manual_seed(0)
    H, W, log = scene['H'], scene['W'], []
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for it in range(iters):
        v = scene['train'][int(torch.randint(0, len(scene['train']), (1,), generator=g, device=device))]
        sel = torch.randint(0, H * W, (4096,), generator=g, device=device)
        rows = ops.ray_rows_from_pose(scene['poses'][v], H, W, scene['focal'], scene['near'], scene['far'], sel=sel)
        r = run.batchify_rays(rows, 1 << 15, **kw)
        tgt = scene['images'][v].reshape(-1, 3)[sel]
        loss = img2mse(r['rgb_map'], tgt) + img2mse(r['rgb0'], tgt)
        if lam > 0:
            loss = loss + lam * (r['dist_loss'] + r['dist_loss0']).mean()
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        for pg in opt.param_groups:
            pg['lr'] = args.lrate * (0.1 ** (it / 250000))
        if it % 500 == 0 or it == iters - 1:
            log.append((it, float(loss.detach())))
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / max(iters, 1) * 1e3
    return dict(te, near=scene['near'], far=scene['far']), ms, log


def evaluate(scene, te, repeats):
    H, W, focal = scene['H'], scene['W'], scene['focal']
    out = {'psnr_heldout': [], 'dist_loss_heldout_mean': []}
    with torch.no_grad():
        for v in HELD:
            rgb, _, _, _, extras = run.render(H, W, focal, chunk=1 << 15, c2w=scene['poses'][v], distortion=True, **te)
            out['psnr_heldout'].append(float(mse2psnr(img2mse(rgb, scene['images'][v]))))
            out['dist_loss_heldout_mean'].append(float(extras['dist_loss'].mean()))
        bmin, bmax = mesh.frustum_bounds(scene['poses'], (H, W, focal), scene['near'], scene['far'])
        grid = OccupancyGrid.from_model(te, bmin, bmax, **GRID)
        out['occupied_fraction'] = grid.occupied_fraction()
        Hh, Wh = HEADLINE
        fh = focal * Wh / W
        frame = lambda occ: run.render(Hh, Wh, fh, chunk=1 << 15, c2w=scene['poses'][HELD[1]], occupancy=occ, **te)
        base, skipped = frame(None)[0], frame(grid)[0]                          # both warmed
        mse = float(((base - skipped) ** 2).mean())
        out['psnr_grid_vs_ordinary'] = None if mse == 0.0 else -10.0 * float(np.log10(mse))
        plain, skip = [], []
        for _ in range(repeats):
            plain.append(event_ms(lambda: frame(None)))
            grid.reset_stats()
            skip.append(event_ms(lambda: frame(grid)))
        s = grid.stats
        out['kept_fraction'] = {'coarse': s['kept_coarse'] / max(1, s['samples_coarse']), 'fine': s['kept_fine'] / max(1, s['samples_fine'])}
        out['ms_frame_ordinary'], out['ms_frame_grid'] = plain, skip
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--iters', type=int, default=1500)
    ap.add_argument('--lambdas', type=float, nargs='+', default=list(LAMBDAS))
    ap.add_argument('--repeats', type=int, default=3)
    a = ap.parse_args(argv)
    dev = torch.device('cuda', 0)
    scene = load_scene(dev)
    out = {'scene': {'fixture': 'tests/golden/scene1_small.npz', 'iterations': a.iters, 'rays_per_iteration': 4096, 'held_out_views': list(HELD),
                     'psnr_frame': [scene['H'], scene['W']], 'timed_frame': list(HEADLINE)},
           'grid': GRID, 'runs': []}
    train(scene, a.lambdas[-1], min(20, a.iters), dev)                          # warm every kernel and the allocator once
    for lam in a.lambdas:
        te, ms, log = train(scene, lam, a.iters, dev)
        run_out = {'distortion_lambda': lam, 'ms_per_iteration': ms, 'loss_log': log}
        run_out.update(evaluate(scene, te, a.repeats))
        out['runs'].append(run_out)
        print(json.dumps(run_out), flush=True)
    base = next((r for r in out['runs'] if r['distortion_lambda'] == 0), None)
    if base is not None:
        for r in out['runs']:
            r['ms_per_iteration_over_lambda_0'] = r['ms_per_iteration'] / base['ms_per_iteration']
    print(json.dumps(out, indent=1))
    out_dir = os.environ.get('MVIP_PROFILE_OUT', 'profile_out')
    os.makedirs(out_dir, exist_ok=True)
    json.dump(out, open(os.path.join(out_dir, 'distortion_ab.json'), 'w'), indent=1)


if __name__ == '__main__':
    main()
