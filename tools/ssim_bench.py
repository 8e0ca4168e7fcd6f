"""Timing of ops.ssim (csrc/ssim.hip) at 378 x 504 x 3 and 1134 x 2016 x 3 (configs[3]'s frame), one image:
the forward alone (no gradient, no map), the forward that also writes the stash, and forward plus backward, against the same
quantity as a torch composition (one grouped conv2d on the five products plus elementwise ops, and its autograd) in the same
process on the same box.

  python tools/ssim_bench.py [--repeats 20] [--out profiles/ssim.json]

Per size: milliseconds between device events around `--inner` back-to-back calls (per call; the median of --repeats windows, the
two implementations alternating), the bytes each launch moves from HBM computed from the shapes (hbm_bytes), what share of the HBM
peak that makes of the measured time, the ratio to the torch composition, and the largest difference between the two results.
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

HBM_PEAK = 8.0e12                    # bytes / s (spec)
COPY_RATE = 6.29e12                  # float4 copy, bytes / s
SIZES = ((378, 504, 3), (1134, 2016, 3))


def hbm_bytes(N, H, W, C, masked=False):
    """Bytes of each launch from the shapes.  E image elements, M map elements, T tiles of 32 x 16 map pixels.  The halo re-reads
    of neighbouring tiles are served by L2 and are not counted."""
    E, M = N * H * W * C, N * (H - 10) * (W - 10) * C
    T = N * (-(-(H - 10) // 16)) * (-(-(W - 10) // 32))
    mask = N * H * W if masked else 0
    return {'forward': 8 * E + mask + 12 * T, 'forward_with_stash': 8 * E + mask + 12 * T + 12 * M, 'reduce': 12 * T + 8 * N,
            'backward': 12 * M + 8 * E + 4 * E}


def torch_ssim(x, y, k2):
    C = x.shape[-1]
    xc, yc = x.permute(0, 3, 1, 2), y.permute(0, 3, 1, 2)
    m = F.conv2d(torch.cat([xc, yc, xc * xc, yc * yc, xc * yc], 1), k2, groups=5 * C)
    mx, my, exx, eyy, exy = m.split(C, 1)
    s = ((2 * mx * my + 1e-4) * (2 * (exy - mx * my) + 9e-4)) / ((mx * mx + my * my + 1e-4) * ((exx - mx * mx) + (eyy - my * my) + 9e-4))
    return s.mean((1, 2, 3))


def window2d(C, dev):
    e = torch.exp(-(torch.arange(11, dtype=torch.float64) - 5.0) ** 2 / 4.5)
    g = (e / e.sum()).float()
    return torch.outer(g, g)[None, None].repeat(5 * C, 1, 1, 1).to(dev)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--repeats', type=int, default=20, help='timed windows per quantity')
    ap.add_argument('--inner', type=int, default=20, help='calls per window')
    ap.add_argument('--out', default=None)
    a = ap.parse_args(argv)
    from mvip_nerf_amd import ops
    dev = torch.device('cuda', 0)

    def window(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.inner):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.inner

    out = {'hbm_peak_bytes_per_s': HBM_PEAK, 'copy_rate_bytes_per_s': COPY_RATE, 'repeats': a.repeats, 'calls_per_window': a.inner,
           'sizes': []}
    for H, W, C in SIZES:
        g = torch.Generator(device='cpu').manual_seed(H)
        y = torch.rand((1, H, W, C), generator=g).to(dev)
        x = (y + 0.05 * torch.randn((1, H, W, C), generator=g).to(dev)).clamp(0, 1).contiguous()
        xg = x.clone().requires_grad_(True)
        k2 = window2d(C, dev)

        def hip_fb():
            xg.grad = None
            ops.ssim(xg, y).sum().backward()

        def torch_fb():
            xg.grad = None
            torch_ssim(xg, y, k2).sum().backward()

        def hip_stash():
            ops.ssim(xg, y)

        runs = {'forward': (lambda: ops.ssim(x, y), lambda: torch_ssim(x, y, k2)),
                'forward_with_stash': (hip_stash, None), 'forward_backward': (hip_fb, torch_fb)}
        hip_fb()
        g_hip = xg.grad.clone()
        torch_fb()
        g_torch = xg.grad.clone()
        row = {'shape': [1, H, W, C], 'bytes_from_shapes': hbm_bytes(1, H, W, C),
               'ssim_hip': float(ops.ssim(x, y)), 'ssim_torch': float(torch_ssim(x, y, k2)),
               'grad_max_abs': float(g_torch.abs().max()), 'grad_max_difference': float((g_hip - g_torch).abs().max())}
        for name, (hip, ref) in runs.items():
            for fn in (hip, ref):                        # warm-up of every shape the timed windows use
                if fn is not None:
                    for _ in range(3):
                        fn()
            torch.cuda.synchronize()
            ms_hip, ms_ref = [], []
            for _ in range(a.repeats):                   # alternating
                ms_hip.append(window(hip))
                if ref is not None:
                    ms_ref.append(window(ref))
            r = {'hip_ms': ms_hip, 'hip_ms_median': float(np.median(ms_hip))}
            if ref is not None:
                r.update(torch_ms=ms_ref, torch_ms_median=float(np.median(ms_ref)),
                         hip_over_torch=float(np.median(ms_hip) / np.median(ms_ref)))
            row[name] = r
        b = row['bytes_from_shapes']
        t_f, t_s, t_fb = (row[k]['hip_ms_median'] * 1e-3 for k in ('forward', 'forward_with_stash', 'forward_backward'))
        # the forward call is two launches (tiles + reduce); the backward's time is the difference of two measured calls
        row['share_of_hbm_peak'] = {'forward_call': (b['forward'] + b['reduce']) / t_f / HBM_PEAK,
                                    'forward_with_stash_call': (b['forward_with_stash'] + b['reduce']) / t_s / HBM_PEAK,
                                    'backward_by_difference': b['backward'] / max(t_fb - t_s, 1e-9) / HBM_PEAK,
                                    'note': 'bytes from shapes over the time of the whole call (launch gaps and torch\'s autograd '
                                            'plumbing included), over the 8.0 TB/s spec; a kernel trace was not taken'}
        out['sizes'].append(row)
    print(json.dumps(out, indent=1))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(out, open(a.out, 'w'), indent=1)
    return 0


if __name__ == '__main__':
    sys.exit(main())
