"""Timing and the cut-out experiment of ops.exemplar_fill (csrc/exemplar.hip) on one GPU.

  python tools/exemplar_bench.py [--repeats 5] --out profiles/exemplar_fill.json

Timing: ms per call (median of --repeats after a warm-up call, between device synchronisations) for the 30 views of
tests/golden/scene1_small.npz (141 x 252) with the dataset's masks, and for one 378 x 504 frame (view 0 with image and mask
upscaled 3 x nearest: the texture is blocky, only the sizes matter), next to ops.harmonic_fill over the three colour planes of
the same masks as the yardstick, and the number of kernel launches of one call, counted from the schedule.

Cut-out experiment: on views 0, 7 and 15 a 24 x 32 hole is cut outside the dataset's mask (view 0: at rows 10 and 100; views 7
and 15: at row 10), the dataset's mask is added to the hole, and inside the cut-out, against the truth that was cut out: the RMS
(in 1 / 255) and the mean absolute horizontal gradient (the texture the fill carries) of the exemplar fill, of the harmonic fill
and of the truth.  Nothing here is a pass / fail figure: the exemplar fill hallucinates texture and is not pixel-accurate.
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

CUTS = ((0, 10), (0, 100), (7, 10), (15, 10))
CUT_H, CUT_W = 24, 32


def launches(levels, rounds=3, iters=4):
    """Kernel launches of one ops.exemplar_fill call whose images use `levels` levels, from the schedule of csrc/exemplar.hip."""
    setup = 2 + 4 * levels + (levels - 1) + 1            # zero + quantise, (row, column, count, scan) per level, the pyramid, the plan
    per_level = 2 + rounds * (iters + 1)                 # initial + vote, rounds x (iters searches + vote)
    return setup + levels + levels * per_level + 1 + 1   # + the lists, + the energy, + the finish


def cut_column(mask, row):
    """The first column at which a CUT_H x CUT_W box at `row` keeps 8 pixels away from the dataset's mask."""
    H, W = mask.shape
    for x in range(8, W - CUT_W - 8):
        if not mask[max(row - 8, 0):row + CUT_H + 8, x - 8:x + CUT_W + 8].any():
            return x
    raise SystemExit(f'no room for a cut-out at row {row}')


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--out', required=True)
    a = ap.parse_args(argv)
    from mvip_nerf_amd import ops
    dev = torch.device('cuda', 0)
    z = np.load(os.path.join(ROOT, 'tests', 'golden', 'scene1_small.npz'), allow_pickle=False)
    images = z['images'].astype(np.float32) / np.float32(255.)
    masks = z['masks'].astype(bool)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)

    def timed(fn):
        fn()
        ms = []
        for _ in range(a.repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        return {'ms': ms, 'ms_median': float(np.median(ms))}

    def planes(img, m):
        N, H, W, _ = img.shape
        return img.permute(0, 3, 1, 2).reshape(3 * N, H, W).contiguous(), m[:, None].expand(N, 3, H, W).reshape(3 * N, H, W).contiguous()

    timing = []
    big = lambda x: np.repeat(np.repeat(x, 3, 1), 3, 2)
    for name, img, m in (('30 views of scene1_small', images, masks), ('one frame, view 0 upscaled 3 x nearest', big(images[:1])[:, :378, :504], big(masks[:1])[:, :378, :504])):
        ti, tm = t(img), t(m)
        _, info = ops.exemplar_fill(ti, tm)
        row = {'case': name, 'images': int(img.shape[0]), 'frame': [int(img.shape[1]), int(img.shape[2])], 'masked_pixels': int(m.sum()),
               'targets': int(info['targets'].sum()), 'levels': info['levels'].tolist(), 'launches_per_call': launches(int(info['levels'].max())),
               'exemplar_fill': timed(lambda: ops.exemplar_fill(ti, tm)),
               'harmonic_fill_three_planes': timed(lambda: ops.harmonic_fill(*planes(ti, tm)))}
        timing.append(row)
    cuts = []
    for view, row in CUTS:
        x = cut_column(masks[view], row)
        m = masks[view].copy()
        cut = np.zeros_like(m)
        cut[row:row + CUT_H, x:x + CUT_W] = True
        m |= cut
        ti, tm = t(images[view:view + 1]), t(m[None])
        ex = ops.exemplar_fill(ti, tm)[0][0].cpu().numpy()
        hp, hm = planes(ti, tm)
        ha = ops.harmonic_fill(hp, hm)[0].reshape(1, 3, *m.shape).permute(0, 2, 3, 1)[0].cpu().numpy()
        truth = images[view]
        box = lambda img: img[row:row + CUT_H, x:x + CUT_W].astype(np.float64) * 255
        rms = lambda img: float(np.sqrt(((box(img) - box(truth)) ** 2).mean()))
        grad = lambda img: float(np.abs(np.diff(box(img), axis=1)).mean())
        cuts.append({'view': view, 'cut_rows': [row, row + CUT_H], 'cut_columns': [x, x + CUT_W],
                     'rms_exemplar': rms(ex), 'rms_harmonic': rms(ha),
                     'gradient_exemplar': grad(ex), 'gradient_harmonic': grad(ha), 'gradient_truth': grad(truth)})
    out = {'what': 'ops.exemplar_fill (DESIGN.md section 18), one GPU: ' + torch.cuda.get_device_name(0),
           'defaults': {'patch': 7, 'rounds': 3, 'iters': 4}, 'repeats': a.repeats, 'timing': timing,
           'cut_out_experiment': {'units': 'RMS and mean |horizontal gradient| in 1 / 255, inside the 24 x 32 cut-out', 'cases': cuts},
           'note': 'recorded, not asserted: the exemplar fill carries texture, it is not pixel-accurate'}
    print(json.dumps(out, indent=1))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(out, open(a.out, 'w'), indent=1)
    return 0


if __name__ == '__main__':
    sys.exit(main())
