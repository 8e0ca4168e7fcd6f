"""Evaluation of rendered views against targets (DS_NeRF/evaluation.py): PSNR, SSIM, L1 / L2, the depth L1 / L2 of its lines
107-108, and the masked and bounding-box variants of the crop its lines 163-169 keep commented out.

PSNR / L1 / L2 are the `img2mse` / `img2l1` / `mse2psnr` expressions in torch.  SSIM is ops.ssim (csrc/ssim.hip): an 11-tap Gaussian
window on every channel, data range 1, no luminance conversion and no downsampling -- NOT pyiqa's Y-channel preprocessing, so
figures are comparable within this project only.  LPIPS and FID need pretrained networks and are not computed.

The host-only helpers (mask_bbox, pair_names, mean_of, write_report, read_report) need no GPU.
"""
import json
import os

import numpy as np
import torch

from .run_nerf_helpers import img2l1, img2mse, mse2psnr

SSIM_MIN_SIDE = 11
IMAGE_EXTENSIONS = ('png', 'jpg', 'jpeg', 'JPG')


# ---- host-only helpers --------------------------------------------------------------------------------------------------------

def mask_bbox(mask):
    """(y0, y1, x0, x1), half-open, of the one rectangle around every set pixel of mask [H, W]; None for an empty mask."""
    m = np.asarray(mask.detach().cpu() if torch.is_tensor(mask) else mask).astype(bool)
    if m.ndim != 2:
        raise ValueError(f'mask_bbox: mask [H, W] expected, got {m.shape}')
    rows, cols = np.flatnonzero(m.any(1)), np.flatnonzero(m.any(0))
    if rows.size == 0:
        return None
    return int(rows[0]), int(rows[-1]) + 1, int(cols[0]), int(cols[-1]) + 1


def pair_names(pred_names, gt_names, what=('predictions', 'targets')):
    """Pair two lists of file names by stem (the name without its extension), in sorted order: [(stem, pred, gt)].  A stem
    without a partner, or one that occurs twice in a list, is an error.  (The reference pairs by os.listdir order, which is
    unspecified.)"""
    def by_stem(names, side):
        out = {}
        for n in names:
            stem = os.path.splitext(os.path.basename(n))[0]
            if stem in out:
                raise ValueError(f'pair_names: {side}: {out[stem]} and {n} share the name {stem}')
            out[stem] = n
        return out
    p, g = by_stem(pred_names, what[0]), by_stem(gt_names, what[1])
    lone = sorted(set(p) - set(g)), sorted(set(g) - set(p))
    if lone[0] or lone[1]:
        raise ValueError(f'pair_names: without a partner: {what[0]} {lone[0]}, {what[1]} {lone[1]}')
    return [(s, p[s], g[s]) for s in sorted(p)]


def mean_of(values):
    """Mean of the entries that are not None (None when there is none)."""
    vals = [float(v) for v in values if v is not None]
    return float(np.mean(vals)) if vals else None


def summarise(per_view):
    """{'per_view': {key: [..]}, 'mean': {key: mean over the views that have the value}, 'views': N}."""
    n = len(next(iter(per_view.values()))) if per_view else 0
    return {'views': n, 'per_view': per_view, 'mean': {k: mean_of(v) for k, v in per_view.items()}}


def write_report(path, report):
    """The report as JSON (indent 1); creates the directory.  Returns the path."""
    d = os.path.dirname(os.path.abspath(path))
    os.makedirs(d, exist_ok=True)
    with open(path, 'w') as f:
        json.dump(report, f, indent=1)
        f.write('\n')
    return path


def read_report(path):
    with open(path) as f:
        return json.load(f)


def _list_images(d):
    return [f for f in sorted(os.listdir(d)) if f.rsplit('.', 1)[-1] in IMAGE_EXTENSIONS and '.' in f]


# ---- metrics --------------------------------------------------------------------------------------------------------------------

def _psnr(mse):
    return float(mse2psnr(mse.reshape(1)))


def image_metrics(pred, gt, mask=None):
    """Per image: dict of lists (length N) psnr, ssim, l1, l2; with mask [N, H, W] bool also psnr_masked (over the masked
    pixels; None for an empty mask), ssim_masked (ops.ssim(..., mask=mask): the map pixels centred on the mask), and psnr_bbox /
    ssim_bbox on the crop to the one rectangle around the whole mask (None for an empty mask; ssim_bbox also None when the crop
    is under 11 pixels in a dimension).  pred, gt [N, H, W, C] fp32 on the GPU in 0..1, C in 1..4; an image under 11 x 11 has
    ssim None."""
    from . import ops
    if not (torch.is_tensor(pred) and torch.is_tensor(gt)) or pred.dim() != 4 or tuple(pred.shape) != tuple(gt.shape):
        shape = lambda t: tuple(t.shape) if torch.is_tensor(t) else type(t).__name__
        raise ValueError(f'image_metrics: pred {shape(pred)} and gt {shape(gt)}: two tensors [N, H, W, C] expected')
    pred, gt = pred.detach().float().contiguous(), gt.detach().float().contiguous()
    N, H, W, C = pred.shape
    if mask is not None:
        if not torch.is_tensor(mask) or mask.dtype != torch.bool or tuple(mask.shape) != (N, H, W):
            raise ValueError(f'image_metrics: mask must be a bool tensor [{N}, {H}, {W}]')
        mask = mask.detach().to(pred.device).contiguous()
    big = H >= SSIM_MIN_SIDE and W >= SSIM_MIN_SIDE
    out = {'psnr': [], 'ssim': ops.ssim(pred, gt).cpu().tolist() if big and N else [None] * N, 'l1': [], 'l2': []}
    for n in range(N):
        mse = img2mse(pred[n], gt[n])
        out['psnr'].append(_psnr(mse))
        out['l1'].append(float(img2l1(pred[n], gt[n])))
        out['l2'].append(float(mse))
    if mask is None:
        return out
    out['ssim_masked'] = ops.ssim(pred, gt, mask=mask).cpu().tolist() if big and N else [None] * N
    out.update(psnr_masked=[], psnr_bbox=[], ssim_bbox=[])
    host = mask.cpu().numpy()
    for n in range(N):
        box = mask_bbox(host[n])
        if box is None:
            for k in ('psnr_masked', 'psnr_bbox', 'ssim_bbox'):
                out[k].append(None)
            continue
        out['psnr_masked'].append(_psnr(img2mse(pred[n][mask[n]], gt[n][mask[n]])))
        y0, y1, x0, x1 = box
        p, g = pred[n:n + 1, y0:y1, x0:x1].contiguous(), gt[n:n + 1, y0:y1, x0:x1].contiguous()
        out['psnr_bbox'].append(_psnr(img2mse(p, g)))
        out['ssim_bbox'].append(float(ops.ssim(p, g)) if min(y1 - y0, x1 - x0) >= SSIM_MIN_SIDE else None)
    return out


def evaluate_views(render_kwargs, hwf, poses, images, near, far, masks=None, disparities=None, chunk=1 << 15):
    """Render every pose [N, 3, 4] without grad (run.render) and compare with images [N, H, W, 3] (image_metrics; masks
    [N, H, W] bool adds the masked and bounding-box values).  With target disparities [N, H, W] the rendered disparity's
    depth_l1 / depth_l2 are added (evaluation.py:107-108).  Returns summarise(...): per-view lists and their means."""
    from . import run
    H, W, focal = int(hwf[0]), int(hwf[1]), float(hwf[2])
    poses = torch.as_tensor(poses)
    if poses.dim() != 3 or tuple(poses.shape[1:]) != (3, 4):
        raise ValueError(f'evaluate_views: poses [N, 3, 4] expected, got {tuple(poses.shape)}')
    N = poses.shape[0]
    images = torch.as_tensor(images)
    if tuple(images.shape) != (N, H, W, 3):
        raise ValueError(f'evaluate_views: images {tuple(images.shape)} for {N} views of {H} x {W}')
    for name, t in (('masks', masks), ('disparities', disparities)):
        if t is not None and tuple(t.shape) != (N, H, W):
            raise ValueError(f'evaluate_views: {name} {tuple(t.shape)} for {N} views of {H} x {W}')
    kw = dict(render_kwargs, near=near, far=far)
    per_view = {}
    with torch.no_grad():
        for n in range(N):
            rgb, disp = run.render(H, W, focal, chunk=int(chunk), c2w=poses[n], **kw)[:2]
            dev = rgb.device
            m = None if masks is None else torch.as_tensor(masks[n:n + 1]).to(dev).bool()
            vals = image_metrics(rgb.reshape(1, H, W, 3), images[n:n + 1].to(dev).float(), m)
            if disparities is not None:
                target = torch.as_tensor(disparities[n]).to(dev).float()
                vals['depth_l1'], vals['depth_l2'] = [float(img2l1(disp, target))], [float(img2mse(disp, target))]
            for k, v in vals.items():
                per_view.setdefault(k, []).extend(v)
    return summarise(per_view)


def mesh_depth_metrics(mesh, hwf, poses, disparities, masks=None, near=1e-3, cull='none'):
    """How far a mesh lies from the depth the renderer sees (beyond the reference, which has no mesh export): the mesh is
    rasterised into every pose [N, 3, >=4] (mesh.render_views, csrc/raster.hip) and its disparity compared with disparities
    [N, H, W] (what prepare.render_disparities returns for the same poses).  Per view and in summary (summarise(...)):
    coverage, the share of the pixels the mesh covers; depth_l1 / depth_l2, img2l1 / img2mse of the two disparities over the
    covered pixels (None where the mesh covers none); with masks [N, H, W] bool also coverage_masked (the share of the mask's
    pixels covered; None for an empty mask) and depth_l1_masked / depth_l2_masked over the covered pixels of the mask."""
    from . import mesh as mesh_mod
    H, W = int(hwf[0]), int(hwf[1])
    dev = mesh.verts.device
    poses = torch.as_tensor(poses)
    if poses.dim() != 3 or poses.shape[1] < 3 or poses.shape[2] < 4:
        raise ValueError(f'mesh_depth_metrics: poses [N, 3, 4] expected, got {tuple(poses.shape)}')
    N = poses.shape[0]
    for name, t in (('disparities', disparities), ('masks', masks)):
        if t is not None and tuple(t.shape) != (N, H, W):
            raise ValueError(f'mesh_depth_metrics: {name} {tuple(t.shape)} for {N} views of {H} x {W}')
    target = torch.as_tensor(disparities).to(dev).float()
    disp, face, _ = mesh_mod.render_views(mesh, hwf, poses, near=near, cull=cull, colors=False)
    covered = face >= 0
    per_view = {'coverage': [], 'depth_l1': [], 'depth_l2': []}
    if masks is not None:
        masks = torch.as_tensor(masks).to(dev).bool()
        per_view.update(coverage_masked=[], depth_l1_masked=[], depth_l2_masked=[])

    def both(sel, n):
        if not bool(sel.any()):
            return None, None
        return float(img2l1(disp[n][sel], target[n][sel])), float(img2mse(disp[n][sel], target[n][sel]))

    for n in range(N):
        per_view['coverage'].append(int(covered[n].sum()) / (H * W))
        l1, l2 = both(covered[n], n)
        per_view['depth_l1'].append(l1)
        per_view['depth_l2'].append(l2)
        if masks is not None:
            m = masks[n]
            per_view['coverage_masked'].append(int((covered[n] & m).sum()) / int(m.sum()) if bool(m.any()) else None)
            l1, l2 = both(covered[n] & m, n)
            per_view['depth_l1_masked'].append(l1)
            per_view['depth_l2_masked'].append(l2)
    return summarise(per_view)


def mesh_image_metrics(mesh, texture, hwf, poses, images, masks=None, near=1e-3, cull='none'):
    """How the exported mesh LOOKS next to images [N, H, W, 3] (uint8, or floats in 0..1) of the cameras poses [N, 3, >=4]
    (beyond the reference, which has no mesh export): the mesh is rendered with `texture` (mesh.render_textured; a
    mesh.Texture) or, with texture None, with its vertex colours (mesh.render_views).  Per view and in summary
    (summarise(...)): coverage, the share of the pixels the mesh covers (of the mask's pixels with masks [N, H, W] bool, which
    then also restricts everything below); psnr over the covered pixels; ssim = ops.ssim with the covered pixels as its mask
    (None for images under 11 x 11).  None where the mesh covers nothing."""
    from . import mesh as mesh_mod, ops
    H, W = int(hwf[0]), int(hwf[1])
    dev = mesh.verts.device
    poses = torch.as_tensor(poses)
    if poses.dim() != 3 or poses.shape[1] < 3 or poses.shape[2] < 4:
        raise ValueError(f'mesh_image_metrics: poses [N, 3, 4] expected, got {tuple(poses.shape)}')
    N = poses.shape[0]
    images = torch.as_tensor(images)
    if tuple(images.shape) != (N, H, W, 3):
        raise ValueError(f'mesh_image_metrics: images {tuple(images.shape)} for {N} views of {H} x {W}')
    if masks is not None and tuple(masks.shape) != (N, H, W):
        raise ValueError(f'mesh_image_metrics: masks {tuple(masks.shape)} for {N} views of {H} x {W}')
    if texture is None:
        if mesh.colors is None:
            raise ValueError('mesh_image_metrics: a mesh without colours needs a texture')
        _, face, rgb = mesh_mod.render_views(mesh, hwf, poses, near=near, cull=cull)
    else:
        _, face, rgb = mesh_mod.render_textured(mesh, texture, hwf, poses, near=near, cull=cull)
    covered = face >= 0
    region = None
    if masks is not None:
        region = torch.as_tensor(masks).to(dev).bool()
        covered = covered & region
    pred = rgb.float() / 255.0
    gt = images.to(dev)
    gt = (gt.float() / 255.0 if gt.dtype == torch.uint8 else gt.float()).contiguous()
    big = H >= SSIM_MIN_SIDE and W >= SSIM_MIN_SIDE
    ssim = ops.ssim(pred.contiguous(), gt, mask=covered.contiguous()).cpu().tolist() if big and N else [None] * N
    per_view = {'coverage': [], 'psnr': [], 'ssim': []}
    for n in range(N):
        total = int(region[n].sum()) if region is not None else H * W
        hit = int(covered[n].sum())
        per_view['coverage'].append(hit / total if total else None)
        per_view['psnr'].append(_psnr(img2mse(pred[n][covered[n]], gt[n][covered[n]])) if hit else None)
        per_view['ssim'].append(ssim[n] if hit else None)
    return summarise(per_view)


def _unit_face_normals(verts, faces):
    """(unit normals [F, 3] fp64, zero for a degenerate face; degenerate [F] bool) on the host: N = (b - a) x (c - a) of the
    widened fp32 vertices, N / sqrt(N . N); degenerate iff not N . N > 0."""
    v = verts.detach().cpu().numpy().astype(np.float64)
    f = faces.detach().cpu().numpy().astype(np.int64)
    with np.errstate(divide='ignore', invalid='ignore'):                              # a NaN vertex: its faces count as degenerate
        u, w = v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]
        N = np.stack([u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1], u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2], u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]], -1)
        nn = (N[:, 0] * N[:, 0] + N[:, 1] * N[:, 1]) + N[:, 2] * N[:, 2]
        bad = ~(nn > 0.0)
        return np.where(bad[:, None], 0.0, N / np.sqrt(nn)[:, None]), bad


def mesh_distance_direction(dist, weights, normals_from, face_of_sample, normals_to, hit_face, thresholds):
    """One direction of mesh_distance_metrics from the samples' distances (host arrays): dist [n] fp32, weights [n] fp64,
    normals_* = _unit_face_normals(...) of the sampled and of the queried mesh, face_of_sample / hit_face [n].  Every sum is
    numpy's sum of the elementwise products in sample order, in fp64 -- a fixed order, so the report is bit-reproducible:
    W = sum(w); mean = sum(w d) / W; rms = sqrt(sum(w d d) / W); max = max(d); within[tau] = sum(w where d <= tau) / W;
    normal_consistency = sum(w |n . n'|) / sum(w) over the samples whose own face and hit face both are non-degenerate."""
    d = np.asarray(dist, np.float32).astype(np.float64)
    w = np.asarray(weights, np.float64)
    W = np.sum(w)
    (nf, bad_f), (nt, bad_t) = normals_from, normals_to
    fos, hit = np.asarray(face_of_sample, np.int64), np.asarray(hit_face, np.int64)
    a, b = nf[fos], nt[hit]
    c = np.abs((a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2])
    wk = np.where(~bad_f[fos] & ~bad_t[hit], w, 0.0)
    with np.errstate(divide='ignore', invalid='ignore'):
        return {'samples': int(len(d)), 'area': float(W), 'mean': float(np.sum(w * d) / W), 'rms': float(np.sqrt(np.sum(w * d * d) / W)),
                'max': float(np.max(d)), 'within': [float(np.sum(np.where(d <= np.float64(t), w, 0.0)) / W) for t in thresholds],
                'normal_consistency': float(np.sum(wk * c) / np.sum(wk))}


def mesh_distance_metrics(mesh_a, mesh_b, samples=2, thresholds=()):
    """How far two triangle meshes lie from each other, over their whole surfaces (beyond the reference, which has no mesh
    export).  mesh_a / mesh_b: mesh.Mesh, or (verts [V, 3] fp32, faces [F, 3] int32) on the GPU.  Each mesh is sampled with
    ops.mesh_sample_faces at subdivision `samples` (samples^2 equal-area points per face, nothing random) and every sample's
    closest point on the other mesh found with ops.mesh_closest_point (csrc/mesh_distance.hip).  The report, a dict:
      a_to_b, b_to_a: {samples, area, mean, rms, max, within [per threshold], normal_consistency} -- area-weighted over the
        samples of the first mesh (mesh_distance_direction);
      chamfer = the mean of the two means; hausdorff = the larger of the two maxima (a sampled Hausdorff distance);
      thresholds; precision = a_to_b's within, recall = b_to_a's, fscore = 2 P R / (P + R) (0 where P + R == 0), per threshold;
      normal_consistency = the mean of the two directions' area-weighted means of |n_a . n_b| (unit fp64 face normals of the
        sample's own face and of the face it hits; degenerate faces excluded on both sides).
    The kernels are deterministic and the reductions run on the host in a fixed order: two calls give the same bits.
    ValueError for samples < 1, a mesh without faces, thresholds that are not finite and >= 0."""
    from . import ops
    import math
    ts = [float(t) for t in thresholds]
    if not all(math.isfinite(t) and t >= 0 for t in ts):
        raise ValueError(f'mesh_distance_metrics: thresholds must be finite and >= 0, got {list(thresholds)!r}')
    pairs = [(m.verts, m.faces) if hasattr(m, 'verts') else (m[0], m[1]) for m in (mesh_a, mesh_b)]
    for v, f in pairs:
        if not torch.is_tensor(f) or f.dim() != 2 or f.shape[0] == 0:
            raise ValueError('mesh_distance_metrics: both meshes need at least one face')
    normals = [_unit_face_normals(v, f) for v, f in pairs]
    grids = [ops.mesh_face_grid(v.detach().contiguous(), f.detach().contiguous()) for v, f in pairs]
    out = []
    for src, dst in ((0, 1), (1, 0)):
        pts, fos, w = ops.mesh_sample_faces(pairs[src][0], pairs[src][1], samples)
        g = grids[dst]
        face, _, dist = ops.mesh_closest_point(pts, g.verts, g.faces, grid=g)
        out.append(mesh_distance_direction(dist.cpu().numpy(), w.cpu().numpy(), normals[src], fos.cpu().numpy(), normals[dst],
                                           face.cpu().numpy(), ts))
    ab, ba = out
    P, R = ab['within'], ba['within']
    return {'thresholds': ts, 'a_to_b': ab, 'b_to_a': ba, 'chamfer': (ab['mean'] + ba['mean']) / 2.0, 'hausdorff': max(ab['max'], ba['max']),
            'precision': list(P), 'recall': list(R), 'fscore': [2.0 * p * r / (p + r) if p + r > 0 else 0.0 for p, r in zip(P, R)],
            'normal_consistency': (ab['normal_consistency'] + ba['normal_consistency']) / 2.0}


def evaluate_folders(pred_dir, gt_dir, mask_dir=None, device=None):
    """The metrics of the images of pred_dir against those of gt_dir (8-bit, read with load_llff._imread, / 255), paired by
    sorted name (pair_names: a name without a partner is an error); mask_dir: one mask per pair (non-zero = masked).  Returns
    summarise(...) with the names added."""
    from .load_llff import _imread
    device = torch.device('cuda', torch.cuda.current_device()) if device is None else device
    pairs = pair_names(_list_images(pred_dir), _list_images(gt_dir))
    mask_of = None
    if mask_dir is not None:
        mask_of = {s: m for s, _, m in pair_names([p for _, p, _ in pairs], _list_images(mask_dir), what=('images', 'masks'))}
    per_view = {}
    load = lambda d, f: torch.from_numpy(np.ascontiguousarray(_imread(os.path.join(d, f))[..., :3]).astype(np.float32) / np.float32(255.))
    for stem, p, g in pairs:
        pred, gt = load(pred_dir, p), load(gt_dir, g)
        if tuple(pred.shape) != tuple(gt.shape):
            raise ValueError(f'evaluate_folders: {p} is {tuple(pred.shape)}, {g} is {tuple(gt.shape)}')
        m = None
        if mask_of is not None:
            raw = np.asarray(_imread(os.path.join(mask_dir, mask_of[stem])))
            raw = raw.reshape(raw.shape[0], raw.shape[1], -1).max(-1)
            if raw.shape != tuple(pred.shape[:2]):
                raise ValueError(f'evaluate_folders: mask {mask_of[stem]} is {raw.shape}, {p} is {tuple(pred.shape[:2])}')
            m = torch.from_numpy(raw != 0)[None].to(device)
        vals = image_metrics(pred[None].to(device), gt[None].to(device), m)
        for k, v in vals.items():
            per_view.setdefault(k, []).extend(v)
    out = summarise(per_view)
    out['names'] = [s for s, _, _ in pairs]
    out['views'] = len(pairs)
    return out
