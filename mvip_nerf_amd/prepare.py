"""Inpainted-depth preparation: the disparity targets of the second stage, made from the field itself (beyond the
reference, which reads them from `Depth_inpainted/*.png` as SPIn-NeRF's `--prepare` render followed by LaMa left them; LaMa
is an external network this repository does not have).

Each training view's disparity is rendered from the field (`render_disparities`) and the masked pixels are replaced by the
HARMONIC interpolant of the pixels around them (`ops.harmonic_fill`: the discrete Laplace equation with the unmasked pixels
as boundary values).  The disparity of a plane is an affine function of the pixel coordinates and affine functions are
harmonic, so a hole in a planar background (floor, wall, table) is reconstructed exactly; a hole that reaches the image
border sees a mirror boundary there and is not.  The definition is csrc/harmonic.hip's and tests/harmonic_numpy.py's.

Who consumes which pixels (scene.build_ray_sets, `LLFFScene(..., inp_pixels=...)`): the depth term of the trainer draws
its rays from `rays_inp`, whose label column is this module's output.  With `inp_pixels='unmasked'` (the default) only the
pixels OUTSIDE the masks are kept: the rendered part of `filled` supervises, the filled part is never read.  With
`'masked'` (SPIn-NeRF's reading) only the pixels inside the masks are kept -- exactly the filled part -- and `'all'` keeps
both.  `prepare_depths(...)['filled'].cpu().numpy()` goes into `scene.LLFFScene(..., inpainted_depths=...)` as it is and
keeps the precision that the 8-bit PNG of `write_llff` drops (one step of 1 / 255).

The third raster, `RGB_inpainted/`, comes from `propagate_reference`: one inpainted view (or a few) is
carried into every other view by backward depth warping (`ops.warp_views`), what no reference sees is filled harmonically,
and `write_images` writes the files.  The inpainted reference itself can be made here too: `inpaint_views` fills the masks of
the reference views with texture from the same image (`ops.exemplar_fill`; plausible, not pixel-accurate),
and `propagate_reference(..., fill='exemplar')` uses the same fill for what no reference sees.  `blend='poisson'` composites in
the gradient domain instead of pasting (`ops.poisson_fill`): the composite's gradients are kept inside each
source, the values come from the view's own pixels around the mask, and the step at the mask edge goes.

Which depth is rendered is a choice: `render_disparities(kind='median')` gives 1 / the median termination
depth of each ray instead of 1 / the expected one, `render_depth_quantiles` several quantiles at once, `spread_mask` the pixels
whose ray sees one thin surface and `consistency_mask` those that other views confirm and none sees through
(`ops.ray_quantile_depth`, `ops.depth_consistency`).  Every default is the expected depth, unfiltered.
"""
import os

import numpy as np
import torch

from . import ops


def _poses(poses):
    poses = torch.as_tensor(poses)
    if poses.dim() != 3 or tuple(poses.shape[1:]) != (3, 4):
        raise ValueError(f'poses [N, 3, 4] expected, got {tuple(poses.shape)}')
    return poses


DEPTH_KINDS = ('expected', 'median')


def _depth_kind(who, kind):
    if kind not in DEPTH_KINDS:
        raise ValueError(f'{who}: kind must be one of {DEPTH_KINDS}, got {kind!r}')
    return kind


def render_disparities(render_kwargs, hwf, poses, near, far, chunk=1 << 15, kind='expected'):
    """float32 [N, H, W] on the device: `disp_map` of a no-grad `run.render` of each pose [N, 3, 4] (camera-to-world), through
    the route of region.propagate_masks; bit-equal to run.render(H, W, focal, chunk=chunk, c2w=pose, near=near, far=far,
    **render_kwargs)[1].  kind='median': 1 / (the median termination depth of the ray) instead, render_depth_quantiles at
    level 0.5 -- 0 where the ray never accumulates half (the median is +inf), NaN where it is NaN; between two surfaces the
    expected depth lies where nothing is, the median on one of them."""
    from . import run
    H, W, focal = int(hwf[0]), int(hwf[1]), float(hwf[2])
    poses = _poses(poses)
    if _depth_kind('render_disparities', kind) == 'median':
        return (1.0 / render_depth_quantiles(render_kwargs, hwf, poses, near, far, (0.5,), chunk)[..., 0]).contiguous()
    kw = dict(render_kwargs, near=near, far=far)
    out = []
    with torch.no_grad():
        for c2w in poses:
            out.append(run.render(H, W, focal, chunk=int(chunk), c2w=c2w, **kw)[1])
    if not out:
        return torch.empty((0, H, W), device=poses.device if poses.is_cuda else 'cuda', dtype=torch.float32)
    return torch.stack(out, 0).contiguous()


def render_depth_quantiles(render_kwargs, hwf, poses, near, far, levels=(0.16, 0.5, 0.84), chunk=1 << 15):
    """float32 [N, H, W, Q] on the device: the 'depth_q' extra of a no-grad `run.render(..., depth_quantiles=levels)` of each
    pose: per pixel the depths at which the ray's accumulated weight reaches each level (ops.ray_quantile_depth; +inf where it
    never does).  The default levels give the median and, as z(0.84) - z(0.16), a thickness: how far the ray is from seeing
    one surface."""
    from . import run
    H, W, focal = int(hwf[0]), int(hwf[1]), float(hwf[2])
    poses = _poses(poses)
    levels = tuple(levels)
    kw = dict(render_kwargs, near=near, far=far, depth_quantiles=levels)
    out = []
    with torch.no_grad():
        for c2w in poses:
            out.append(run.render(H, W, focal, chunk=int(chunk), c2w=c2w, **kw)[4]['depth_q'])
    if not out:
        return torch.empty((0, H, W, len(levels)), device=poses.device if poses.is_cuda else 'cuda', dtype=torch.float32)
    return torch.stack(out, 0).contiguous()


def spread_mask(depth_q, max_spread):
    """bool [N, H, W]: the pixels of depth_q [N, H, W, 3] (levels low < mid < high, e.g. render_depth_quantiles' default) whose
    three quantiles are finite and whose relative thickness (z_high - z_low) / z_mid is <= max_spread."""
    if not torch.is_tensor(depth_q) or depth_q.dim() != 4 or depth_q.shape[-1] != 3:
        raise ValueError(f'spread_mask: depth_q [N, H, W, 3] expected, got '
                         f'{tuple(depth_q.shape) if torch.is_tensor(depth_q) else type(depth_q).__name__}')
    max_spread = float(max_spread)
    if not 0.0 <= max_spread < float('inf'):
        raise ValueError(f'spread_mask: max_spread must be finite and >= 0, got {max_spread}')
    lo, mid, hi = depth_q[..., 0], depth_q[..., 1], depth_q[..., 2]
    return torch.isfinite(depth_q).all(-1) & ((hi - lo) / mid <= max_spread)


def consistency_mask(disp, poses, focal, tol=0.05, min_agree=1, max_violated=0, masks=None):
    """bool [N, H, W]: the pixels of disp [N, H, W] that at least `min_agree` other views confirm and at most `max_violated`
    other views see through (ops.depth_consistency; `masks` as there).  The defaults keep what one other camera has seen
    at the same place and no camera has seen through.  A pixel without a finite disparity > 0 counts 0 / 0."""
    min_agree, max_violated = int(min_agree), int(max_violated)
    if min_agree < 0 or max_violated < 0:
        raise ValueError(f'consistency_mask: min_agree {min_agree} and max_violated {max_violated} must be >= 0')
    poses = _poses(poses)
    if torch.is_tensor(disp) and poses.device != disp.device:
        poses = poses.to(disp.device)
    agree, violated = ops.depth_consistency(disp, poses.to(torch.float32).contiguous(), focal, masks=masks, tol=tol)
    return (agree >= min_agree) & (violated <= max_violated)


def prepare_depths(render_kwargs, hwf, poses, masks, near, far, dilate=0, chunk=1 << 15, allow_unconverged=False, kind='expected',
                   **fill_kw):
    """Render the disparity of every pose and fill the masked pixels harmonically.  masks [N, H, W] bool (tensor or array);
    `dilate` rounds of ops.mask_dilate2d are applied first (a generous mask keeps the object's rim out of the boundary
    values); fill_kw goes to ops.harmonic_fill (eps, max_iters, check_every); `kind` is render_disparities' ('median': the
    median termination depth instead of the expected one).

    Returns dict(disp [N, H, W] the rendered disparity, filled [N, H, W], masks [N, H, W] bool: the dilated set that was
    filled, info: ops.harmonic_fill's).  Non-finite rendered pixels are filled too.  ValueError for a singular view (every
    pixel masked or non-finite: nothing to interpolate from); RuntimeError naming the views that did not converge within
    max_iters, unless allow_unconverged."""
    H, W = int(hwf[0]), int(hwf[1])
    poses = _poses(poses)
    if _depth_kind('prepare_depths', kind) == 'expected':
        disp = render_disparities(render_kwargs, hwf, poses, near, far, chunk)
    else:
        disp = render_disparities(render_kwargs, hwf, poses, near, far, chunk, kind=kind)
    masks = torch.as_tensor(np.asarray(masks) if not torch.is_tensor(masks) else masks)
    if tuple(masks.shape) != (poses.shape[0], H, W):
        raise ValueError(f'masks [{poses.shape[0]}, {H}, {W}] expected, got {tuple(masks.shape)}')
    masks = ops.mask_dilate2d((masks != 0).to(disp.device), dilate)
    filled, info = ops.harmonic_fill(disp, masks, **fill_kw)
    singular = np.nonzero(info['singular'])[0].tolist()
    if singular:
        raise ValueError(f'prepare_depths: views {singular} have no known pixel (fully masked or not finite)')
    bad = np.nonzero(~info['converged'])[0].tolist()
    if bad and not allow_unconverged:
        raise RuntimeError(f'prepare_depths: views {bad} did not converge in {info["iterations"][bad].tolist()} iterations '
                           f'(raise max_iters, or pass allow_unconverged=True)')
    return {'disp': disp, 'filled': filled, 'masks': masks, 'info': info}


def write_llff(root, names, masks, depths):
    """Write root/label/NAME.png (0 / 255) and root/Depth_inpainted/NAME.png (round(clip(d, 0, 1) * 255)), grey in all three
    channels: the layout load_llff._load_data reads (it takes channel 0 and divides by 255).  masks / depths [N, H, W]
    (tensors or arrays).  Returns the number of depth pixels that were clipped (outside [0, 1], or not finite: written as 0)."""
    from . import run
    masks = masks.detach().cpu().numpy() if torch.is_tensor(masks) else np.asarray(masks)
    depths = depths.detach().cpu().numpy() if torch.is_tensor(depths) else np.asarray(depths)
    names = list(names)
    if masks.ndim != 3 or masks.shape != depths.shape or masks.shape[0] != len(names):
        raise ValueError(f'masks {masks.shape} and depths {depths.shape} for {len(names)} names: [N, H, W] of one shape expected')
    os.makedirs(os.path.join(root, 'label'), exist_ok=True)
    os.makedirs(os.path.join(root, 'Depth_inpainted'), exist_ok=True)
    d = depths.astype(np.float64)
    finite = np.isfinite(d)
    clipped = int((~finite | (d < 0) | (d > 1)).sum())
    d8 = np.round(np.clip(np.where(finite, d, 0.0), 0.0, 1.0) * 255.0).astype(np.uint8)
    m8 = (masks != 0).astype(np.uint8) * 255
    grey = lambda a: np.ascontiguousarray(np.repeat(a[..., None], 3, -1))
    for i, name in enumerate(names):
        run._write_png(os.path.join(root, 'label', name + '.png'), grey(m8[i]))
        run._write_png(os.path.join(root, 'Depth_inpainted', name + '.png'), grey(d8[i]))
    return clipped


# ---- reference-view propagation: the RGB_inpainted/ images from one inpainted view (or a few) ---------------------------------------

def _to_device(a, device, dtype):
    t = a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))
    return t.detach().to(device=device, dtype=dtype).contiguous()


def reference_order(poses, ref_views):
    """int32 [N, R]: per view the positions in ref_views ordered by the distance between the camera centres (fp64 on the host),
    ties by position."""
    c = np.asarray(poses, np.float64)[:, :3, 3]
    dist = np.linalg.norm(c[:, None, :] - c[None, list(ref_views), :], axis=-1)
    return np.argsort(dist, axis=1, kind='stable').astype(np.int32)


FILLS = {True: 'harmonic', False: 'none', 'harmonic': 'harmonic', 'exemplar': 'exemplar', 'none': 'none'}


def inpaint_views(images, masks, views, method='exemplar', **kw):
    """The `ref_images` of propagate_reference made from the dataset alone: images[views] with their masks filled by
    ops.exemplar_fill (kw: patch, rounds, iters, seed, sources, max_levels).  images [N, H, W, 3] fp32 in 0..1, masks [N, H, W]
    bool (tensors or arrays; the work is done on the device of `images` when that is a GPU tensor, else on 'cuda').  Returns
    [len(views), H, W, 3] on the device.  ValueError for an unknown method, bad views, and a view with no exemplar."""
    if method != 'exemplar':
        raise ValueError(f'inpaint_views: method {method!r}: \'exemplar\' expected')
    shape = lambda a: tuple(a.shape) if hasattr(a, 'shape') else type(a).__name__
    if len(shape(images)) != 4 or shape(images)[-1] != 3:
        raise ValueError(f'inpaint_views: images [N, H, W, 3] expected, got {shape(images)}')
    N, H, W, _ = shape(images)
    if shape(masks) != (N, H, W):
        raise ValueError(f'inpaint_views: masks {shape(masks)} for images {shape(images)}: [{N}, {H}, {W}] expected')
    views = [int(v) for v in views]
    if not views or min(views) < 0 or max(views) >= N:
        raise ValueError(f'inpaint_views: views {views}: at least one view of 0..{N - 1} expected')
    device = images.device if torch.is_tensor(images) and images.is_cuda else torch.device('cuda')
    pick = lambda a: a[views] if not torch.is_tensor(a) else a[torch.as_tensor(views, device=a.device)]
    img = _to_device(pick(images), device, torch.float32)
    msk = (torch.as_tensor(np.asarray(pick(masks)) if not torch.is_tensor(masks) else pick(masks)) != 0).to(device).contiguous()
    if kw.get('sources') is not None:
        s = kw['sources']
        kw = dict(kw, sources=(torch.as_tensor(np.asarray(pick(s)) if not torch.is_tensor(s) else pick(s)) != 0).to(device).contiguous())
    filled, info = ops.exemplar_fill(img, msk, **kw)
    singular = [views[i] for i in np.nonzero(info['singular'])[0]]
    if singular:
        raise ValueError(f'inpaint_views: views {singular} have no exemplar (no patch free of masked pixels)')
    return filled


def propagate_reference(images, masks, disparities, poses, focal, ref_views, ref_images=None, tol=0.05, fill=True, blend='none',
                        **fill_kw):
    """Carry the inpainted reference views into every other view through geometry (beyond the reference, whose RGB_inpainted/
    images are independent 2D inpaintings): each masked pixel is lifted with its own disparity and looks its colour up in
    the nearest reference view that sees the same surface (ops.warp_views; the definition is csrc/warp.hip's).

    images [N, H, W, 3] fp32 in 0..1, masks [N, H, W] bool, disparities [N, H, W] (the field's: prepare_depths(...)['filled'];
    or the dataset's rasters; nothing is rendered here), poses [N, 3, 4], ref_views: indices of the inpainted views,
    ref_images [R, H, W, 3]: their inpainted images (None: images[ref_views]).  Tensors or arrays; the work is done on the
    device of `images` when that is a GPU tensor, else on 'cuda'.

    Per target the references are tried in the order of reference_order.  The output image is `images` outside the mask bit
    for bit, the warped colour where a reference was taken, and on the remaining masked pixels (holes) the harmonic
    interpolant of the pixels around them, per channel, by one ops.harmonic_fill call over [3N, H, W] (fill=False leaves
    `images` there; fill_kw: eps, max_iters, check_every, and allow_unconverged as in prepare_depths).  fill='exemplar' fills
    the holes with texture instead: one ops.exemplar_fill call over the N views with the holes as its masks and
    sources = the pixels outside that view's mask, so that exemplars come from original pixels only (fill_kw: patch, rounds,
    iters, seed, max_levels); 'harmonic' and 'none' are the names of True and False.  A view that is itself a
    reference takes its reference image unchanged (its masked pixels name itself as the source).

    Returns dict(images [N, H, W, 3], source [N, H, W] int32: -1 or the position in ref_views, resid [N, H, W], holes
    [N, H, W] bool = masks & (source < 0), coverage: numpy [N], the share of each view's masked pixels with a source (1 for
    an empty mask), info: ops.harmonic_fill's over the planes 3 n + channel, ops.exemplar_fill's over the views for
    fill='exemplar', None without fill).  ValueError for mismatched shapes, an unknown fill, an empty or invalid ref_views, and
    a plane (a view) with nothing to interpolate (copy) from; RuntimeError naming the views whose
    fill did not converge, unless allow_unconverged.

    blend='poisson' composites in the gradient domain instead of pasting (Perez, Gangnet, Blake 2003; ops.poisson_fill, the
    definition is csrc/harmonic.hip's): the composite above becomes a GUIDE whose differences are kept, and the values come from
    the view's own pixels around the mask.  It needs fill 'harmonic' or 'exemplar' (the solve fills the holes anyway).  The warp
    runs over the masks dilated by one pixel, so that the ring just outside a mask carries a guide colour and a source too;
    source, resid, holes and coverage are reported on the masks alone and are blend='none''s.  Labels are the source over the
    dilated region and -1 elsewhere: a difference is kept only between two pixels of one reference, and across a change of
    reference, at a hole, and where the ring found no reference the edge is harmonic.  With fill='exemplar' the holes' exemplar
    texture enters the guide under a label of its own, len(ref_views).  The unknowns are the whole mask of every
    non-reference view, the boundary values the original images; one ops.poisson_fill call over [3N, H, W] (fill_kw's eps,
    max_iters, check_every go to it).  The dict gains 'pasted', the images of blend='none'; info is ops.poisson_fill's over
    the planes 3 n + channel.  Blended values may leave [0, 1]: nothing clamps them here (write_images clips and counts).
    ValueError for an unknown blend and for blend='poisson' with fill='none'."""
    if blend not in ('none', 'poisson'):
        raise ValueError(f'propagate_reference: blend {blend!r}: \'none\' or \'poisson\' expected')
    if isinstance(fill, str) and fill not in FILLS:
        raise ValueError(f'propagate_reference: fill {fill!r}: True / \'harmonic\', \'exemplar\' or False / \'none\' expected')
    fill = FILLS[fill if isinstance(fill, str) else bool(fill)]
    if blend == 'poisson' and fill == 'none':
        raise ValueError('propagate_reference: blend \'poisson\' fills the holes by its solve: fill \'harmonic\' or \'exemplar\' expected')
    allow_unconverged = bool(fill_kw.pop('allow_unconverged', False))
    device = images.device if torch.is_tensor(images) and images.is_cuda else torch.device('cuda')
    shape = lambda a: tuple(a.shape) if hasattr(a, 'shape') else type(a).__name__
    if len(shape(images)) != 4 or shape(images)[-1] != 3:
        raise ValueError(f'propagate_reference: images [N, H, W, 3] expected, got {shape(images)}')
    N, H, W, _ = shape(images)
    if shape(masks) != (N, H, W) or shape(disparities) != (N, H, W):
        raise ValueError(f'propagate_reference: masks {shape(masks)} and disparities {shape(disparities)} for images {shape(images)}: '
                         f'[{N}, {H}, {W}] expected')
    poses_t = _poses(poses)
    if poses_t.shape[0] != N:
        raise ValueError(f'propagate_reference: {poses_t.shape[0]} poses for {N} images')
    refs = [int(v) for v in ref_views]
    if not refs or len(set(refs)) != len(refs) or min(refs) < 0 or max(refs) >= N:
        raise ValueError(f'propagate_reference: ref_views {refs}: at least one view of 0..{N - 1}, each once, expected')
    if ref_images is not None and shape(ref_images) != (len(refs), H, W, 3):
        raise ValueError(f'propagate_reference: ref_images {shape(ref_images)}: [{len(refs)}, {H}, {W}, 3] expected')
    img = _to_device(images, device, torch.float32)
    msk = (torch.as_tensor(np.asarray(masks) if not torch.is_tensor(masks) else masks) != 0).to(device).contiguous()
    disp = _to_device(disparities, device, torch.float32)
    pose = _to_device(poses_t, device, torch.float32)
    ridx = torch.as_tensor(refs, device=device, dtype=torch.int64)
    src_rgb = _to_device(ref_images, device, torch.float32) if ref_images is not None else img[ridx].contiguous()
    order = torch.from_numpy(reference_order(pose.cpu().numpy(), refs)).to(device)
    warp_mask = msk.clone()
    warp_mask[ridx] = False                                   # a reference view is not warped into
    wide = None
    if blend == 'poisson':
        wide = ops.mask_dilate2d(warp_mask, 1)                # the masks and the ring just outside them; empty for a reference view
        solver_kw = {k: fill_kw[k] for k in ('eps', 'max_iters', 'check_every') if k in fill_kw}
        if fill == 'exemplar':
            fill_kw = {k: v for k, v in fill_kw.items() if k not in solver_kw}
    rgb, source, resid = ops.warp_views(disp, pose, warp_mask if wide is None else wide, src_rgb, disp[ridx].contiguous(), pose[ridx].contiguous(),
                                        float(focal), order=order.contiguous(), tol=tol)
    if wide is not None:                                      # a per-pixel gather: on the masks it is the warp over the masks
        rgb_wide, source_wide = rgb, source
        zero = torch.zeros((), device=device)
        rgb, resid = torch.where(warp_mask[..., None], rgb, zero), torch.where(warp_mask, resid, zero)
        source = torch.where(warp_mask, source, torch.full((), -1, device=device, dtype=source.dtype))
    out = torch.where((source >= 0)[..., None], rgb, img)
    for k, v in enumerate(refs):
        out[v] = src_rgb[k]
        source[v] = torch.where(msk[v], k, -1).to(source.dtype)
    holes = msk & (source < 0)
    info = None
    if fill == 'exemplar':
        out, info = ops.exemplar_fill(out.contiguous(), holes.contiguous(), sources=(~msk).contiguous(), **fill_kw)
        singular = np.nonzero(info['singular'])[0].tolist()
        if singular:
            raise ValueError(f'propagate_reference: views {singular} have no exemplar outside their masks to fill their holes from')
    elif fill == 'harmonic':
        planes = out.permute(0, 3, 1, 2).reshape(3 * N, H, W).contiguous()
        filled, info = ops.harmonic_fill(planes, holes[:, None].expand(N, 3, H, W).reshape(3 * N, H, W).contiguous(), **fill_kw)
        singular = sorted({int(p) // 3 for p in np.nonzero(info['singular'])[0]})
        if singular:
            raise ValueError(f'propagate_reference: views {singular} have no known pixel to fill their holes from')
        bad = sorted({int(p) // 3 for p in np.nonzero(~info['converged'])[0]})
        if bad and not allow_unconverged:
            raise RuntimeError(f'propagate_reference: the fill of views {bad} did not converge (raise max_iters, or pass '
                               f'allow_unconverged=True)')
        out = torch.where(holes[..., None], filled.reshape(N, 3, H, W).permute(0, 2, 3, 1), out)
    n_mask = msk.sum((1, 2)).cpu().numpy().astype(np.float64)
    n_src = (msk & (source >= 0)).sum((1, 2)).cpu().numpy().astype(np.float64)
    coverage = np.where(n_mask > 0, n_src / np.maximum(n_mask, 1.0), 1.0)
    result = {'images': out.contiguous(), 'source': source, 'resid': resid, 'holes': holes, 'coverage': coverage, 'info': info}
    if wide is None:
        return result
    pasted = result['images']
    labels = source_wide.clone()                              # -1 off the dilated region: the warp leaves it so
    guide = rgb_wide
    if fill == 'exemplar':
        labels[holes] = len(refs)
        guide = torch.where(holes[..., None], pasted, guide)
    planes = lambda a: a.permute(0, 3, 1, 2).reshape(3 * N, H, W).contiguous()
    over_channels = lambda a: a[:, None].expand(N, 3, H, W).reshape(3 * N, H, W).contiguous()
    filled, info = ops.poisson_fill(planes(img), over_channels(warp_mask), planes(guide), over_channels(labels), **solver_kw)
    singular = sorted({int(p) // 3 for p in np.nonzero(info['singular'])[0]})
    if singular:
        raise ValueError(f'propagate_reference: views {singular} have no known pixel to blend their masks from')
    bad = sorted({int(p) // 3 for p in np.nonzero(~info['converged'])[0]})
    if bad and not allow_unconverged:
        raise RuntimeError(f'propagate_reference: the blend of views {bad} did not converge (raise max_iters, or pass '
                           f'allow_unconverged=True)')
    blended = torch.where(warp_mask[..., None], filled.reshape(N, 3, H, W).permute(0, 2, 3, 1), img)
    for k, v in enumerate(refs):
        blended[v] = src_rgb[k]
    result.update(images=blended.contiguous(), pasted=pasted, info=info)
    return result


def write_images(root, names, images):
    """Write root/RGB_inpainted/NAME.png (round(clip(v, 0, 1) * 255)): the images load_llff._load_data reads.  images
    [N, H, W, 3] (tensor or array).  Returns the number of values that were clipped (outside [0, 1], or not finite: written
    as 0)."""
    from . import run
    images = images.detach().cpu().numpy() if torch.is_tensor(images) else np.asarray(images)
    names = list(names)
    if images.ndim != 4 or images.shape[-1] != 3 or images.shape[0] != len(names):
        raise ValueError(f'images {images.shape} for {len(names)} names: [N, H, W, 3] expected')
    os.makedirs(os.path.join(root, 'RGB_inpainted'), exist_ok=True)
    v = images.astype(np.float64)
    finite = np.isfinite(v)
    clipped = int((~finite | (v < 0) | (v > 1)).sum())
    v8 = np.round(np.clip(np.where(finite, v, 0.0), 0.0, 1.0) * 255.0).astype(np.uint8)
    for i, name in enumerate(names):
        run._write_png(os.path.join(root, 'RGB_inpainted', name + '.png'), np.ascontiguousarray(v8[i]))
    return clipped
