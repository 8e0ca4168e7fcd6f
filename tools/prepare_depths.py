"""Inpainted-depth targets from the field itself (mvip_nerf_amd/prepare.py): render every view's disparity, dilate the masks,
fill the masked pixels with the harmonic interpolant of the pixels around them, write the layout the loader reads.

  python tools/prepare_depths.py --fixture [--dilate 2] --out DIR
  python tools/prepare_depths.py --checkpoint CKPT.tar --datadir SCENE [--factor 4] [--dilate 2] --out DIR

--fixture trains the scene-1 fixture (tests/golden/scene1_small.npz, the 1,500-iteration recipe of
tools/render_occupancy_ab.py::train_scene1) and uses the fixture's own masks; --checkpoint / --datadir load a model in the
reference's .tar format and a SPIn-NeRF style scene with its label/*.png (the routes of tools/propagate_masks.py).

Into DIR: label/NAME.png (0 / 255, the dilated masks that were filled), Depth_inpainted/NAME.png (round(clip(d, 0, 1) * 255)),
filled.npy (float32 [N, H, W]: what scene.LLFFScene(..., inpainted_depths=...) takes without the 8-bit rounding), and one JSON
(printed, and DIR/depth_prepare.json): per-view unknowns, iterations and true residual, seconds per stage, clipped pixels.
With --fixture also the comparison with the dataset's own (LaMa-inpainted) rasters: RMS of rendered-and-filled disparity
against them inside and outside the masks, and of the fill applied to the dataset's rasters themselves.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def rms255(a, b, sel):
    return float(np.sqrt(((a[sel].astype(np.float64) - b[sel]) ** 2).mean()) * 255.0) if sel.any() else 0.0


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--fixture', action='store_true')
    ap.add_argument('--iters', type=int, default=1500, help='training iterations of --fixture')
    ap.add_argument('--checkpoint')
    ap.add_argument('--datadir')
    ap.add_argument('--factor', type=int, default=4)
    ap.add_argument('--dilate', type=int, default=0, help='rounds of 2D dilation of the masks before the fill')
    ap.add_argument('--eps', type=float, default=1e-7)
    ap.add_argument('--max-iters', type=int, default=None)
    ap.add_argument('--depth', choices=('expected', 'median'), default='expected',
                    help='render the expected ray depth (default) or the median termination depth')
    ap.add_argument('--out', required=True)
    a = ap.parse_args(argv)
    if a.fixture == bool(a.checkpoint) or bool(a.checkpoint) != bool(a.datadir):
        ap.error('either --fixture, or --checkpoint with --datadir')
    from mvip_nerf_amd import ops, prepare
    from tools import propagate_masks as P
    dev = torch.device('cuda', 0)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return out, time.perf_counter() - t0

    (te, hwf, poses, masks, valid, names, near, far, source), t_model = timed(
        lambda: P.fixture_scene(dev, a.iters) if a.fixture else P.checkpoint_scene(dev, a.checkpoint, a.datadir, a.factor))
    if not valid.all():
        raise SystemExit(f'views {np.nonzero(~valid)[0].tolist()} have no mask')
    os.makedirs(a.out, exist_ok=True)
    disp, t_render = timed(lambda: prepare.render_disparities(te, hwf, poses, near, far, kind=a.depth))
    dil, t_dilate = timed(lambda: ops.mask_dilate2d(torch.from_numpy(masks).to(dev), a.dilate))
    (filled, info), t_fill = timed(lambda: ops.harmonic_fill(disp, dil, eps=a.eps, max_iters=a.max_iters))
    if info['singular'].any() or not info['converged'].all():
        raise SystemExit(f'singular views {np.nonzero(info["singular"])[0].tolist()}, unconverged views '
                         f'{np.nonzero(~info["converged"])[0].tolist()}')
    f_np, d_np, m_np = filled.cpu().numpy(), disp.cpu().numpy(), dil.cpu().numpy()
    clipped, t_write = timed(lambda: prepare.write_llff(a.out, names, m_np, f_np))
    np.save(os.path.join(a.out, 'filled.npy'), f_np)
    total = t_render + t_dilate + t_fill + t_write
    out = {'source': source, 'frame': [hwf[0], hwf[1]], 'views': len(names), 'dilate': a.dilate, 'eps': a.eps, 'depth': a.depth,
           'mask_share_of_frame': float(masks.mean()), 'filled_share_of_frame': float(m_np.mean()),
           'unknowns_per_view': info['unknowns'].tolist(), 'iterations_per_view': info['iterations'].tolist(),
           'true_residual_per_view': [float(r) for r in info['residual']], 'clipped_pixels': clipped,
           'non_finite_rendered_pixels': int((~np.isfinite(d_np)).sum()),
           'seconds': {'model': t_model, 'render': t_render, 'dilate': t_dilate, 'fill': t_fill, 'write': t_write},
           'render_share_of_prepare': t_render / total}
    if a.fixture:
        data = np.load(os.path.join(ROOT, 'tests', 'golden', 'scene1_small.npz'))['depths'].astype(np.float32) / np.float32(255.)
        own, _ = ops.harmonic_fill(torch.from_numpy(data).to(dev), dil)
        own = own.cpu().numpy()
        out['against_dataset_rasters_rms_255'] = {
            'note': 'the field was trained on already-inpainted images (DESIGN section 12); the dataset rasters are LaMa output',
            'rendered_and_filled_inside_masks': float(np.mean([rms255(f_np[v], data[v], m_np[v]) for v in range(len(names))])),
            'rendered_outside_masks': float(np.mean([rms255(f_np[v], data[v], ~m_np[v]) for v in range(len(names))])),
            'rendered_unfilled_inside_masks': float(np.mean([rms255(np.nan_to_num(d_np[v]), data[v], m_np[v]) for v in range(len(names))])),
            'dataset_rasters_filled_inside_masks': float(np.mean([rms255(own[v], data[v], m_np[v]) for v in range(len(names))]))}
    print(json.dumps(out, indent=1))
    json.dump(out, open(os.path.join(a.out, 'depth_prepare.json'), 'w'), indent=1)
    return 0


if __name__ == '__main__':
    sys.exit(main())
