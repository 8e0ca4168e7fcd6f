"""Evaluate renders against targets (mvip_nerf_amd/evaluate.py; DS_NeRF/evaluation.py): PSNR, SSIM, L1 / L2 per view and their
means, with masks also over the masked pixels and on the crop to the mask's bounding rectangle.

  python tools/evaluate.py --checkpoint CKPT.tar --datadir SCENE [--factor 4] [--views 0,5,10] [--out report.json]
  python tools/evaluate.py --pred DIR --gt DIR [--masks DIR] [--out report.json]

The first form renders the views of a SPIn-NeRF style scene (load_llff_data: RGB_inpainted/, label/, Depth_inpainted/) from a
checkpoint in the reference's .tar format and compares them with the scene's images, inside the scene's masks, and the rendered
disparity with the scene's depth rasters (depth_l1 / depth_l2).  The second compares two folders of 8-bit images paired by sorted
name; a name without a partner is an error.  SSIM here is an 11-tap Gaussian window per channel at data range 1 with no luminance
conversion: not pyiqa's Y-channel preprocessing.  LPIPS and FID are not computed (they need pretrained networks).  The report is
printed as JSON and written to --out.
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


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--checkpoint', help='model in the reference\'s .tar format')
    ap.add_argument('--datadir', help='LLFF scene directory (with --checkpoint)')
    ap.add_argument('--factor', type=int, default=4)
    ap.add_argument('--model', choices=('mlp', 'tcnn'), default='mlp')
    ap.add_argument('--views', default=None, help='comma separated view indices (default: all)')
    ap.add_argument('--chunk', type=int, default=1 << 15)
    ap.add_argument('--pred', help='folder of predicted images')
    ap.add_argument('--gt', help='folder of target images')
    ap.add_argument('--masks', help='folder of masks (with --pred / --gt; non-zero = masked)')
    ap.add_argument('--out', default=None, help='write the report here as JSON')
    a = ap.parse_args(argv)
    folders, field = bool(a.pred or a.gt), bool(a.checkpoint or a.datadir)
    if folders == field:
        ap.error('either --checkpoint and --datadir, or --pred and --gt')
    if folders and not (a.pred and a.gt):
        ap.error('--pred and --gt go together')
    if field and not (a.checkpoint and a.datadir):
        ap.error('--checkpoint and --datadir go together')
    from mvip_nerf_amd import evaluate
    dev = torch.device('cuda', 0)
    if folders:
        report = evaluate.evaluate_folders(a.pred, a.gt, a.masks, device=dev)
        report['source'] = {'pred': a.pred, 'gt': a.gt, 'masks': a.masks}
    else:
        from mvip_nerf_amd.load_llff import load_llff_data
        from tools.extract_mesh import load_model
        images, poses, bds, _, _, masks, depths, mask_indices = load_llff_data(a.datadir, factor=a.factor)
        H, W, focal = (float(v) for v in poses[0, :3, -1])
        views = list(range(len(images))) if a.views is None else [int(v) for v in a.views.split(',') if v != '']
        have_masks = len(mask_indices) == len(images)
        kw, step = load_model(a.checkpoint, a.model, dev)
        report = evaluate.evaluate_views(
            kw, (int(H), int(W), focal), torch.from_numpy(np.ascontiguousarray(poses[views, :3, :4]).astype(np.float32)).to(dev),
            torch.from_numpy(images[views][..., :3].astype(np.float32)), float(bds.min() * .9), float(bds.max()),
            masks=torch.from_numpy(np.asarray(masks)[views] == 1) if have_masks else None,
            disparities=torch.from_numpy(np.asarray(depths)[views].astype(np.float32)) if len(depths) == len(images) else None,
            chunk=a.chunk)
        report['source'] = {'checkpoint': a.checkpoint, 'global_step': step, 'datadir': a.datadir, 'factor': a.factor, 'view_indices': views}
    print(json.dumps(report, indent=1))
    if a.out:
        evaluate.write_report(a.out, report)
    return 0


if __name__ == '__main__':
    sys.exit(main())
