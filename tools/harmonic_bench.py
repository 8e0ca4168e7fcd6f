"""Timing of ops.harmonic_fill at frame size: batches of 60 views at 1128 x 2016 and 564 x 1008 made from the
scene-1 fixture's masks and depth rasters upscaled x 8 and x 4 (masks nearest, depth bilinear; the 30 views twice).

  python tools/harmonic_bench.py [--out profiles/depth_prepare.json] [--host-solve]
  python tools/harmonic_bench.py --once 8          # one fill at x 8 and nothing else: the run to put under a kernel trace

Per size: milliseconds of one fill between device events (the median of --repeats), iterations per view, unknowns and
active 64 x 16 tiles per view, the bytes an iteration moves computed from the shapes (46 B per pixel of an active tile: stencil
1 + 8 read + 8 written, update 1 + 16 read + 12 written) and the rate that makes of the time.  --host-solve adds the scipy
direct solve of one view on the host for context.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FIXTURE = os.path.join(ROOT, 'tests', 'golden', 'scene1_small.npz')
BYTES_PER_TILE_PIXEL = 46
COPY_RATE = 6.29e12                  # float4 copy, bytes / s


def batch(scale, views, dev):
    z = np.load(FIXTURE)
    d = torch.from_numpy(z['depths'].astype(np.float32) / np.float32(255.))[:, None]
    m = torch.from_numpy(z['masks'].astype(np.float32))[:, None]
    H, W = d.shape[2] * scale, d.shape[3] * scale
    d = F.interpolate(d, size=(H, W), mode='bilinear', align_corners=False)[:, 0]
    m = F.interpolate(m, size=(H, W), mode='nearest')[:, 0] > 0.5
    reps = (views + d.shape[0] - 1) // d.shape[0]
    return d.repeat(reps, 1, 1)[:views].contiguous().to(dev), m.repeat(reps, 1, 1)[:views].contiguous().to(dev)


def active_tiles(m):
    N, H, W = m.shape
    p = F.pad(m, (0, (-W) % 64, 0, (-H) % 16))
    return p.reshape(N, p.shape[1] // 16, 16, p.shape[2] // 64, 64).any(4).any(2).sum((1, 2))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--views', type=int, default=60)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--once', type=int, default=None, metavar='SCALE')
    ap.add_argument('--host-solve', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args(argv)
    from mvip_nerf_amd import ops
    dev = torch.device('cuda', 0)
    if a.once is not None:
        d, m = batch(a.once, a.views, dev)
        _, info = ops.harmonic_fill(d, m)
        torch.cuda.synchronize()
        print(json.dumps({'scale': a.once, 'iterations_max': int(info['iterations'].max()), 'converged': bool(info['converged'].all())}))
        return 0
    out = {'views': a.views, 'source': 'tests/golden/scene1_small.npz, masks nearest and depth bilinear upscaled', 'sizes': []}
    for scale in (4, 8):
        d, m = batch(scale, a.views, dev)
        ops.harmonic_fill(d[:2], m[:2])                                         # load the library, warm the allocator
        ms = []
        for _ in range(a.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            filled, info = ops.harmonic_fill(d, m)
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        one = []
        for _ in range(a.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            _, info1 = ops.harmonic_fill(d[:1], m[:1])
            e1.record()
            torch.cuda.synchronize()
            one.append(e0.elapsed_time(e1))
        tiles = active_tiles(m).cpu().numpy()
        it = info['iterations']
        launched = int(-(-it.max() // 32) * 32)                                 # the flags are read back every 32 iterations
        bytes_per_iteration_all = float(tiles.sum()) * 1024 * BYTES_PER_TILE_PIXEL
        bytes_moved = float((tiles * it).sum()) * 1024 * BYTES_PER_TILE_PIXEL    # a frozen view moves nothing
        t = float(np.median(ms)) * 1e-3
        rec = {'frame': [int(d.shape[1]), int(d.shape[2])], 'ms_fill_batch': ms, 'ms_fill_batch_median': float(np.median(ms)),
               'ms_fill_single_view': one, 'ms_per_view_in_batch': float(np.median(ms)) / a.views,
               'iterations_per_view': it.tolist(), 'iterations_launched': launched, 'launches': 2 * launched + 5,
               'unknowns_per_view': info['unknowns'].tolist(), 'active_tiles_per_view': tiles.tolist(),
               'converged': bool(info['converged'].all()), 'true_residual_max': float(info['residual'].max()),
               'bytes_per_iteration_all_views_live': bytes_per_iteration_all, 'bytes_moved_total': bytes_moved,
               'hbm_rate_bytes_per_s': bytes_moved / t, 'share_of_copy_rate': bytes_moved / t / COPY_RATE,
               'us_per_launch': t / (2 * launched + 5) * 1e6,
               'workspace_bytes': int(ops._lib.load().mvip_harmonic_workspace_bytes(a.views, d.shape[1], d.shape[2]))}
        if a.host_solve:
            sys.path.insert(0, os.path.join(ROOT, 'tests'))
            import harmonic_numpy as R
            t0 = time.perf_counter()
            f64, _ = R.solve(d[0].cpu().numpy(), m[0].cpu().numpy())
            rec['host_scipy_direct_solve_one_view_s'] = time.perf_counter() - t0
            U = m[0].cpu().numpy()
            rec['gpu_against_host_solve_max_error'] = float(np.abs(filled[0].cpu().numpy().astype(np.float64) - f64)[U].max())
        out['sizes'].append(rec)
        del d, m, filled
    print(json.dumps(out, indent=1))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(out, open(a.out, 'w'), indent=1)
    return 0


if __name__ == '__main__':
    sys.exit(main())
