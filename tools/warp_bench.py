"""Timing of ops.warp_views at frame size: 60 targets of 564 x 1008 made from the scene-1 fixture's images,
masks and disparity rasters upscaled x 4 (bilinear; masks nearest; the 30 views twice, the focal length x 4), warped from 1 source
(view 0) and from 3 (views 0, 15, 29, ordered per target by camera distance), with the dataset's masks and with every pixel masked.

  python tools/warp_bench.py [--out FILE.json]
  python tools/warp_bench.py --once 3 [--full-mask]     # one warm-up and one warp with 3 sources: the run to put under a kernel trace

Per configuration: milliseconds of one warp between device events (the median of --repeats), the share of masked pixels that took
a source, the bytes the kernel moves from HBM computed from the shapes (hbm_bytes) and the rate that makes of the time.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FIXTURE = os.path.join(ROOT, 'tests', 'golden', 'scene1_small.npz')
COPY_RATE = 6.29e12                  # float4 copy, bytes / s
REFS = {1: [0], 3: [0, 15, 29]}


def hbm_bytes(N, H, W, S):
    """Bytes of one warp from the shapes: every target pixel's disparity and mask read (5 B) and its colour, index and residual
    written (20 B); each source's disparity and colour (16 B per pixel) fetched once -- the targets' gathers revisit them
    through L2 and the Infinity Cache, which hold S frames of 16 B x H x W (9.1 MB each at 564 x 1008)."""
    return N * H * W * 25 + S * H * W * 16


def batch(scale, views, dev):
    z = np.load(FIXTURE)
    up = lambda a, mode: F.interpolate(a, scale_factor=scale, mode=mode, **({} if mode == 'nearest' else {'align_corners': False}))
    img = up(torch.from_numpy(z['images'].astype(np.float32) / np.float32(255.)).permute(0, 3, 1, 2), 'bilinear').permute(0, 2, 3, 1)
    d = up(torch.from_numpy(z['depths'].astype(np.float32) / np.float32(255.))[:, None], 'bilinear')[:, 0]
    m = up(torch.from_numpy(z['masks'].astype(np.float32))[:, None], 'nearest')[:, 0] > 0.5
    pose = torch.from_numpy(np.ascontiguousarray(z['poses'][:, :, :4]))
    focal = float(z['poses'][0, 2, 4]) * m.shape[2] / float(z['poses'][0, 1, 4])
    reps = (views + d.shape[0] - 1) // d.shape[0]
    rep = lambda a: a.repeat(reps, *([1] * (a.dim() - 1)))[:views].contiguous().to(dev)
    return rep(img), rep(d), rep(m), rep(pose), focal


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--views', type=int, default=60)
    ap.add_argument('--scale', type=int, default=4)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--once', type=int, default=None, choices=sorted(REFS), metavar='SOURCES')
    ap.add_argument('--full-mask', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args(argv)
    from mvip_nerf_amd import ops, prepare
    dev = torch.device('cuda', 0)
    img, d, m, pose, focal = batch(a.scale, a.views, dev)
    N, H, W = d.shape

    def operands(S, full):
        refs = REFS[S]
        order = torch.from_numpy(prepare.reference_order(pose.cpu().numpy(), refs)).to(dev).contiguous()
        mask = torch.ones_like(m) if full else m
        return (d, pose, mask, img[refs].contiguous(), d[refs].contiguous(), pose[refs].contiguous(), focal), order, mask

    if a.once is not None:
        args, order, mask = operands(a.once, a.full_mask)
        ops.warp_views(*args, order=order)
        _, index, _ = ops.warp_views(*args, order=order)
        torch.cuda.synchronize()
        print(json.dumps({'sources': a.once, 'full_mask': a.full_mask, 'frame': [H, W], 'views': N,
                          'taken_share_of_masked': float((index >= 0).sum()) / float(mask.sum())}))
        return 0
    out = {'views': N, 'frame': [H, W], 'source': 'tests/golden/scene1_small.npz upscaled, masks nearest, images and disparities bilinear',
           'copy_rate_bytes_per_s': COPY_RATE, 'runs': []}
    for S in sorted(REFS):
        for full in (False, True):
            args, order, mask = operands(S, full)
            ops.warp_views(*args, order=order)
            ms = []
            for _ in range(a.repeats):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                _, index, _ = ops.warp_views(*args, order=order)
                e1.record()
                torch.cuda.synchronize()
                ms.append(e0.elapsed_time(e1))
            t, nbytes = float(np.median(ms)) * 1e-3, hbm_bytes(N, H, W, S)
            out['runs'].append({'sources': S, 'every_pixel_masked': full, 'masked_share_of_frame': float(mask.float().mean()),
                                'taken_share_of_masked': float((index >= 0).sum()) / float(mask.sum()),
                                'sources_taken': torch.bincount(index[index >= 0].flatten(), minlength=S).tolist(),
                                'ms': ms, 'ms_median': float(np.median(ms)), 'bytes_from_shapes': nbytes,
                                'rate_bytes_per_s': nbytes / t, 'share_of_copy_rate': nbytes / t / COPY_RATE})
    print(json.dumps(out, indent=1))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(out, open(a.out, 'w'), indent=1)
    return 0


if __name__ == '__main__':
    sys.exit(main())
