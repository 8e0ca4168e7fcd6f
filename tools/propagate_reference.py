"""Reference-view propagation (mvip_nerf_amd/prepare.py): carry one inpainted view (or a few) into every other view by backward
depth warping, fill what no reference sees harmonically, write the RGB_inpainted/ images the loader reads.

  python tools/propagate_reference.py --fixture [--ref-views 0] [--tol 0.05] --out DIR
  python tools/propagate_reference.py --datadir SCENE [--factor 4] --ref-views 0,30 [--ref-image A.png --ref-image B.png] --out DIR
  ... --depths field --checkpoint CKPT.tar      (the field's disparities, prepare.prepare_depths, instead of the dataset's rasters)
  ... --inpaint exemplar [--fill exemplar]      (the reference images made here: prepare.inpaint_views, no network and no weights)
  ... --blend poisson                           (gradient-domain compositing instead of pasting: ops.poisson_fill)

--fixture uses tests/golden/scene1_small.npz (images, masks, 8-bit disparity rasters, poses); --datadir a SPIn-NeRF style scene
with its RGB_inpainted/, label/ and Depth_inpainted/.  --ref-image replaces the image of a reference view, in the order of
--ref-views (a 2D inpainting made elsewhere); without it the scene's own image of that view is the reference, or with
--inpaint exemplar that image with its mask filled by ops.exemplar_fill (texture copied from the rest of the image: plausible,
not pixel-accurate).  --fill says what goes into the pixels no reference sees: the harmonic interpolant (the default), the
exemplar fill (from pixels outside the view's mask), or nothing.  --depths field
renders the disparities from a model instead (--checkpoint in the reference's .tar format; with --fixture and no checkpoint
the 1,500-iteration recipe of tools/render_occupancy_ab.py::train_scene1 is trained first) and fills them inside the masks.

Into DIR: RGB_inpainted/NAME.png, source.npy (int32 [N, H, W]: -1 or the position in --ref-views), and one JSON (printed, and
DIR/reference_propagation.json): per view the coverage (share of the masked pixels that found a reference), the RMS inside the
mask against the scene's own images (all masked pixels, and the warped ones alone), the same for the baseline that fills the
whole mask harmonically, a sweep over tol, and seconds per stage.

--blend poisson (prepare.propagate_reference(blend='poisson')) writes the blended images instead of the
pasted ones, and the JSON gains `blend`: per view and as a mean over the non-reference views the BOUNDARY STEP (mean
|x_p - x_q| over the mask's boundary edges, p in the mask and q its 4-neighbour outside, over the three channels) of the pasted
composite, of the blended result and of the scene's own image on the same edges (the natural level), the RMS inside the mask
of both against the scene's images, the solver's iteration counts, and the seconds of the blended call beside the pasted one
and the baseline fill (the same unknowns with a zero guide).  Every other key is about the pasted composite, as without it.
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

SWEEP = (0.01, 0.02, 0.05, 0.1, 0.2)


def rms(a, b, sel):
    return float(np.sqrt(((a[sel].astype(np.float64) - b[sel]) ** 2).mean())) if sel.any() else None


def boundary_step(x, mask):
    """Mean |x_p - x_q| over the boundary edges of mask [H, W] (p inside, q a 4-neighbour outside) and the channels of x
    [H, W, 3]; None without such an edge."""
    x = x.astype(np.float64)
    total, count = 0.0, 0
    for inner, outer in ((np.s_[1:, :], np.s_[:-1, :]), (np.s_[:-1, :], np.s_[1:, :]), (np.s_[:, 1:], np.s_[:, :-1]), (np.s_[:, :-1], np.s_[:, 1:])):
        edge = mask[inner] & ~mask[outer]
        total += float(np.abs(x[inner][edge] - x[outer][edge]).sum())
        count += int(edge.sum()) * x.shape[-1]
    return total / count if count else None


def load_scene(a, dev):
    """(images [N,H,W,3], masks, dataset disparities, poses [N,3,4], (H, W, focal), names, near, far) as numpy."""
    if a.fixture:
        z = np.load(os.path.join(ROOT, 'tests', 'golden', 'scene1_small.npz'), allow_pickle=False)
        images = z['images'].astype(np.float32) / np.float32(255.)
        H, W = images.shape[1:3]
        focal = float(z['poses'][0, 2, 4]) * W / float(z['poses'][0, 1, 4])
        names = ['{:06d}'.format(i) for i in range(len(images))]
        return images, z['masks'].astype(bool), z['depths'].astype(np.float32) / np.float32(255.), \
            np.ascontiguousarray(z['poses'][:, :, :4]), (H, W, focal), names, float(z['bds'].min() * .9), float(z['bds'].max())
    from mvip_nerf_amd.load_llff import load_llff_data
    images, poses, bds, _, _, masks, depths, mask_indices = load_llff_data(a.datadir, factor=a.factor)
    if len(mask_indices) != len(images):
        raise SystemExit(f'{a.datadir}: {len(mask_indices)} masks for {len(images)} views: one per view expected')
    H, W, focal = (float(v) for v in poses[0, :3, -1])
    root = os.path.join(a.datadir, 'images' if a.factor is None else f'images_{a.factor}', 'RGB_inpainted')
    names = [f.split('.')[0] for f in sorted(os.listdir(root)) if f.endswith(('JPG', 'jpg', 'jpeg', 'png'))]
    return images.astype(np.float32), masks == 1, depths.astype(np.float32), np.ascontiguousarray(poses[:, :3, :4]).astype(np.float32), \
        (int(H), int(W), focal), names, float(bds.min() * .9), float(bds.max())


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--fixture', action='store_true')
    ap.add_argument('--datadir')
    ap.add_argument('--factor', type=int, default=4)
    ap.add_argument('--ref-views', default='0', help='the inpainted views, comma separated (default 0)')
    ap.add_argument('--ref-image', action='append', default=[], metavar='PNG',
                    help='the inpainted image of a reference view, in the order of --ref-views; may be repeated')
    ap.add_argument('--inpaint', choices=('none', 'exemplar'), default='none',
                    help='make the reference images without a --ref-image here: exemplar = prepare.inpaint_views')
    ap.add_argument('--fill', choices=('harmonic', 'exemplar', 'none'), default='harmonic', help='what fills the pixels no reference sees')
    ap.add_argument('--blend', choices=('none', 'poisson'), default='none',
                    help='poisson: keep the composite\'s gradients and take the values from the view\'s own pixels around the mask')
    ap.add_argument('--tol', type=float, default=0.05, help='relative depth tolerance of the visibility test')
    ap.add_argument('--depths', choices=('dataset', 'field'), default='dataset')
    ap.add_argument('--checkpoint', help='model for --depths field')
    ap.add_argument('--iters', type=int, default=1500, help='training iterations of --fixture --depths field without a checkpoint')
    ap.add_argument('--out', required=True)
    a = ap.parse_args(argv)
    if a.fixture == bool(a.datadir):
        ap.error('either --fixture or --datadir')
    if a.depths == 'field' and not a.fixture and not a.checkpoint:
        ap.error('--depths field needs --checkpoint (or --fixture)')
    refs = [int(v) for v in a.ref_views.split(',') if v != '']
    if len(a.ref_image) > len(refs):
        ap.error('more --ref-image than --ref-views')
    if a.blend == 'poisson' and a.fill == 'none':
        ap.error('--blend poisson needs --fill harmonic or exemplar')
    from mvip_nerf_amd import load_llff, ops, prepare
    dev = torch.device('cuda', 0)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return out, time.perf_counter() - t0

    (images, masks, data_disp, poses, hwf, names, near, far), t_load = timed(lambda: load_scene(a, dev))
    N, H, W = masks.shape
    seconds = {'load': t_load}
    disp = torch.from_numpy(data_disp).to(dev)
    if a.depths == 'field':
        if a.checkpoint:
            from tools.extract_mesh import load_model
            (kw, _), seconds['model'] = timed(lambda: load_model(a.checkpoint, 'mlp', dev))
            te = dict(kw, near=near, far=far)
        else:
            from tools import render_occupancy_ab as T
            scene, seconds['model'] = timed(lambda: T.train_scene1(dev, a.iters))
            te = scene['te']
        out, seconds['depths'] = timed(lambda: prepare.prepare_depths(te, hwf, torch.from_numpy(poses).to(dev), masks, near, far))
        disp = out['filled']
    ref_images = images[refs].copy()
    if a.inpaint == 'exemplar' and len(a.ref_image) < len(refs):
        made, seconds['inpaint'] = timed(lambda: prepare.inpaint_views(images, masks, refs[len(a.ref_image):]))
        ref_images[len(a.ref_image):] = made.cpu().numpy()
    for k, path in enumerate(a.ref_image):
        png = load_llff._imread(path)[..., :3].astype(np.float32) / np.float32(255.)
        if png.shape != (H, W, 3):
            raise SystemExit(f'{path}: {png.shape[0]} x {png.shape[1]}, the scene is {H} x {W}')
        ref_images[k] = png
    img_t, msk_t, pose_t = torch.from_numpy(images).to(dev), torch.from_numpy(masks).to(dev), torch.from_numpy(poses).to(dev)
    run = lambda tol, fill, blend='none': prepare.propagate_reference(img_t, msk_t, disp, pose_t, hwf[2], refs, ref_images=ref_images, tol=tol,
                                                                      fill=fill, blend=blend)
    _, seconds['warp_and_fill_first_call'] = timed(lambda: run(a.tol, a.fill))
    res, seconds['warp_and_fill'] = timed(lambda: run(a.tol, a.fill))
    _, seconds['warp'] = timed(lambda: run(a.tol, 'none'))
    got, source = res['images'].cpu().numpy(), res['source'].cpu().numpy()
    blended = None
    if a.blend == 'poisson':
        _, seconds['warp_fill_and_blend_first_call'] = timed(lambda: run(a.tol, a.fill, 'poisson'))
        res_b, seconds['warp_fill_and_blend'] = timed(lambda: run(a.tol, a.fill, 'poisson'))
        blended = res_b['images'].cpu().numpy()
        if not np.array_equal(res_b['pasted'].cpu().numpy().view(np.int32), got.view(np.int32)):
            raise SystemExit('the pasted composite of blend=poisson differs from blend=none')
    os.makedirs(a.out, exist_ok=True)
    clipped, seconds['write'] = timed(lambda: prepare.write_images(a.out, names, got if blended is None else blended))
    np.save(os.path.join(a.out, 'source.npy'), source)
    # the baseline: no reference at all, the whole mask filled harmonically per channel
    planes = img_t.permute(0, 3, 1, 2).reshape(3 * N, H, W).contiguous()
    mask_planes = msk_t[:, None].expand(N, 3, H, W).reshape(3 * N, H, W).contiguous()
    (base, base_info), seconds['baseline_fill'] = timed(lambda: ops.harmonic_fill(planes, mask_planes))
    base = base.reshape(N, 3, H, W).permute(0, 2, 3, 1).cpu().numpy()
    others = [v for v in range(N) if v not in refs]
    warped = masks & (source >= 0)
    per_view = lambda img, sel: [rms(img[v], images[v], sel[v]) for v in range(N)]
    mean = lambda xs: float(np.mean([x for v, x in enumerate(xs) if v in others and x is not None])) if others else None
    in_mask, in_warped, baseline = per_view(got, masks), per_view(got, warped), per_view(base, masks)
    sweep = []
    for tol in SWEEP:
        r = run(tol, a.fill)
        g, s = r['images'].cpu().numpy(), r['source'].cpu().numpy()
        sweep.append({'tol': tol, 'mean_coverage': float(np.mean(r['coverage'][others])) if others else None,
                      'min_coverage': float(np.min(r['coverage'][others])) if others else None,
                      'mean_rms_in_mask': mean(per_view(g, masks)), 'mean_rms_warped_pixels': mean(per_view(g, masks & (s >= 0)))})
    out = {'scene': 'tests/golden/scene1_small.npz' if a.fixture else a.datadir, 'frame': [H, W], 'views': N, 'ref_views': refs,
           'ref_images': a.ref_image, 'inpaint': a.inpaint, 'fill': a.fill, 'depths': a.depths, 'tol': a.tol, 'mask_share_of_frame': float(masks.mean()),
           'coverage_per_view': [float(c) for c in res['coverage']], 'holes_per_view': res['holes'].sum((1, 2)).cpu().tolist(),
           'rms_in_mask_per_view': in_mask, 'rms_warped_pixels_per_view': in_warped, 'rms_baseline_harmonic_fill_per_view': baseline,
           'mean_over_non_reference_views': {'coverage': float(np.mean(res['coverage'][others])) if others else None,
                                             'rms_in_mask': mean(in_mask), 'rms_warped_pixels': mean(in_warped),
                                             'rms_baseline_harmonic_fill': mean(baseline)},
           'note': 'RMS in 0..1 against the scene\'s own images (independent 2D inpaintings of every view) inside the masks',
           'fill_iterations_max': int(res['info']['iterations'].max()) if a.fill == 'harmonic' else None, 'clipped_values': clipped, 'tol_sweep': sweep, 'seconds': seconds}
    if blended is not None:
        step = lambda img: [boundary_step(img[v], masks[v]) if v in others else None for v in range(N)]
        steps = {'pasted': step(got), 'blended': step(blended), 'scene_image': step(images)}
        rms_b = per_view(blended, masks)
        its = res_b['info']['iterations'].reshape(N, 3)
        median5 = lambda fn: float(np.median([timed(fn)[1] for _ in range(5)]))          # every shape has run before: warm
        base_its = base_info['iterations'].reshape(N, 3)
        out['blend'] = {
            'method': 'poisson', 'boundary_step_per_view': steps, 'rms_in_mask_per_view': {'pasted': in_mask, 'blended': rms_b},
            'iterations_per_view': its.max(1).tolist(), 'baseline_fill_iterations_per_view': base_its.max(1).tolist(),
            'mean_over_non_reference_views': {'boundary_step_pasted': mean(steps['pasted']), 'boundary_step_blended': mean(steps['blended']),
                                              'boundary_step_scene_image': mean(steps['scene_image']),
                                              'rms_in_mask_pasted': mean(in_mask), 'rms_in_mask_blended': mean(rms_b)},
            'iterations_max': int(its[others].max()) if others else None,
            'baseline_fill_iterations_max': int(base_its[others].max()) if others else None,
            'seconds_median_of_5': {'blended_call': median5(lambda: run(a.tol, a.fill, 'poisson')), 'pasted_call': median5(lambda: run(a.tol, a.fill)),
                                    'baseline_fill': median5(lambda: ops.harmonic_fill(planes, mask_planes))},
            'values_outside_0_1': int(((blended < 0) | (blended > 1)).sum()),
            'note': 'boundary step: mean |x_p - x_q| over the edges from a masked pixel p to its unmasked 4-neighbour q, three channels; '
                    'scene_image is the step the scene\'s own image has on the same edges.  The images written are the blended ones'}
    print(json.dumps(out, indent=1))
    json.dump(out, open(os.path.join(a.out, 'reference_propagation.json'), 'w'), indent=1)
    return 0


if __name__ == '__main__':
    sys.exit(main())
