"""What `region=` costs (mvip_nerf_amd/region.py, csrc/region.hip), on the bench frame (378 x 504, 64 + 64 samples, random-weight
model), in ONE process.

  python tools/region_bench.py [--repeats 5]      frames with and without `region=` alternated, device events around whole
                                                  frames; prints one JSON (and $MVIP_PROFILE_OUT/region_bench.json)
  python tools/region_bench.py --kernel-only      20 launches of the accumulate pass alone on one frame's rows, depths and
                                                  weights (128 samples per ray), for `rocprofv3 --kernel-trace --stats`; prints
                                                  the bytes the pass has to move: 8 B per sample + 44 B per ray + 4 B out
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

import bench                                                                  # noqa: E402
from mvip_nerf_amd import ops, run                                            # noqa: E402
from mvip_nerf_amd.region import Region                                       # noqa: E402
from tools.render_occupancy_ab import event_ms                                # noqa: E402

CELLS = (64, 64, 64)
BOX = ((-1.5, -1.2, -4.3), (1.5, 1.2, -0.7))            # depths 1.0 .. 4.6 in front of bench.orbit_pose(0)


def ball_region(device, radius=0.3):
    ax = [(np.arange(c) + 0.5) / c - 0.5 for c in CELLS]
    X, Y, Z = np.meshgrid(*ax, indexing='ij')
    bits = np.zeros(ops.occupancy_words(CELLS) * 32, np.uint8)
    bits[:X.size] = (X * X + Y * Y + Z * Z <= radius * radius).reshape(-1)
    words = np.packbits(bits.reshape(-1, 32), axis=1, bitorder='little').reshape(-1).view('<u4').view(np.int32)
    return Region(BOX[0], BOX[1], CELLS, torch.from_numpy(words.copy()).to(device))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--kernel-only', action='store_true')
    a = ap.parse_args(argv)
    dev = torch.device('cuda', 0)
    region = ball_region(dev)
    pose = bench.orbit_pose(0, dev)
    if a.kernel_only:
        rows = ops.ray_rows_from_pose(pose, bench.H, bench.W, bench.FOCAL, bench.NEAR, bench.FAR)
        B, S = rows.shape[0], 128
        z = ops.stratified_z(rows, S, True)
        w = torch.rand((B, S), device=dev) / S
        for _ in range(20):
            out = ops.region_accumulate(rows, z, w, region.box(), region.cells, region.words)
        torch.cuda.synchronize()
        print(json.dumps({'rays': B, 'samples_per_ray': S, 'bytes_per_launch': B * S * 8 + B * 44 + B * 4, 'launches': 20,
                          'mean_share_inside': float(out.mean() / w.sum(1).mean())}))
        return 0
    torch.manual_seed(0)
    _, te, *_ = run.create_nerf(bench.make_args(), device=dev)
    kw = dict(te, near=bench.NEAR, far=bench.FAR)

    def frame(r):
        with torch.no_grad():
            return run.render(bench.H, bench.W, bench.FOCAL, chunk=1 << 15, c2w=pose, region=r, **kw)
    frame(None), frame(region)
    plain, with_region = [], []
    for _ in range(a.repeats):
        plain.append(event_ms(lambda: frame(None)))
        with_region.append(event_ms(lambda: frame(region)))
    n_chunks = -(-bench.H * bench.W // (1 << 15))
    S = kw['N_samples'] + kw['N_importance']
    out = {'frame': [bench.H, bench.W], 'samples_final_pass': S, 'chunks': n_chunks, 'extra_launches_per_frame': n_chunks,
           'extra_bytes_per_frame': bench.H * bench.W * (S * 8 + 48), 'ms_plain': plain, 'ms_with_region': with_region,
           'ms_plain_spread': max(plain) - min(plain), 'ms_difference_of_means': float(np.mean(with_region) - np.mean(plain))}
    print(json.dumps(out, indent=1))
    out_dir = os.environ.get('MVIP_PROFILE_OUT', 'profile_out')
    os.makedirs(out_dir, exist_ok=True)
    json.dump(out, open(os.path.join(out_dir, 'region_bench.json'), 'w'), indent=1)
    return 0


if __name__ == '__main__':
    sys.exit(main())
