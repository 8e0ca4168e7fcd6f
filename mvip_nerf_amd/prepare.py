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


def render_disparities(render_kwargs, hwf, poses, near, far, chunk=1 << 15):
    """float32 [N, H, W] on the device: `disp_map` of a no-grad `run.render` of each pose [N, 3, 4] (camera-to-world), through
    the route of region.propagate_masks; bit-equal to run.render(H, W, focal, chunk=chunk, c2w=pose, near=near, far=far,
    **render_kwargs)[1]."""
    from . import run
    H, W, focal = int(hwf[0]), int(hwf[1]), float(hwf[2])
    poses = _poses(poses)
    kw = dict(render_kwargs, near=near, far=far)
    out = []
    with torch.no_grad():
        for c2w in poses:
            out.append(run.render(H, W, focal, chunk=int(chunk), c2w=c2w, **kw)[1])
    if not out:
        return torch.empty((0, H, W), device=poses.device if poses.is_cuda else 'cuda', dtype=torch.float32)
    return torch.stack(out, 0).contiguous()


def prepare_depths(render_kwargs, hwf, poses, masks, near, far, dilate=0, chunk=1 << 15, allow_unconverged=False, **fill_kw):
    """Render the disparity of every pose and fill the masked pixels harmonically.  masks [N, H, W] bool (tensor or array);
    `dilate` rounds of ops.mask_dilate2d are applied first (a generous mask keeps the object's rim out of the boundary
    values); fill_kw goes to ops.harmonic_fill (eps, max_iters, check_every).

    Returns dict(disp [N, H, W] the rendered disparity, filled [N, H, W], masks [N, H, W] bool: the dilated set that was
    filled, info: ops.harmonic_fill's).  Non-finite rendered pixels are filled too.  ValueError for a singular view (every
    pixel masked or non-finite: nothing to interpolate from); RuntimeError naming the views that did not converge within
    max_iters, unless allow_unconverged."""
    H, W = int(hwf[0]), int(hwf[1])
    poses = _poses(poses)
    disp = render_disparities(render_kwargs, hwf, poses, near, far, chunk)
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
