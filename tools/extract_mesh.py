"""Triangle mesh of a trained model: load a checkpoint in the reference's .tar format (what run.save_checkpoint writes,
`module.` key prefixes accepted), sample sigma on a grid inside a box, run marching cubes, colour the vertices and write a
binary PLY (mvip_nerf_amd/mesh.py).  Prints sigma percentiles of the grid (to choose --threshold) and each stage's time.

  python tools/extract_mesh.py CKPT.tar --out mesh.ply [--model mlp|tcnn] [--bound-min x y z --bound-max x y z]
         [--resolution 256] [--threshold 10] [--network fine|coarse] [--precision fp32|split] [--no-colors]
         [--keep-largest K] [--min-component N] [--smooth ITERS] [--simplify STEPS] [--simplify-placement quadric|mean]
         [--drop-interior K] [--drop-unseen --datadir SCENE [--factor 4]] [--texture N [--texture-from render|dataset] --out mesh.obj]
         [--mesh-largest K] [--mesh-min-faces N] [--close-holes N] [--report-topology] [--report-error]
         [--save-region R.npz] [--save-occupancy O.npz] [--grid-cells 128] [--grid-dilate 1]
  python tools/extract_mesh.py --tsdf --fixture [--iters 1500] --out mesh.ply [--trunc T] [--view-step S] ...
  python tools/extract_mesh.py --tsdf CKPT.tar --datadir SCENE [--factor 4] --out mesh.ply [--trunc T] [--view-step S] ...

--keep-largest K keeps the K largest connected components of the inside lattice points, --min-component N those of at
least N points (mesh.remove_floaters, connectivity 6; both: a component must meet both); the counts before and after are
printed.

--smooth ITERS runs ITERS Taubin iterations on the extracted mesh (mesh.smooth; 0, the default: off), --simplify STEPS then
clusters its vertices in cubic cells of STEPS times the largest lattice step (mesh.simplify, --simplify-placement quadric or
mean; 0, the default: off).  Both come after the floater options and recompute the normals from the faces; the colours are
those of the extracted vertices (averaged per cluster).  The triangle and vertex counts before and after are printed.
Without the two flags the file is what it was.

--drop-unseen rasterises the finished mesh into the training cameras (mesh.visible_faces, csrc/raster.hip) and writes only
the faces that win a pixel in at least one of them, with the vertices those faces use: the interior sheets and back shells
of a sigma level set go.  It comes last, after the clean-up.  The cameras are those of --tsdf; without --tsdf they are read
from --datadir / --factor.  Without the flag the file is what it was.

--drop-interior K casts K spherical-Fibonacci directions (1..255) from every face of the finished mesh (mesh.drop_interior,
csrc/mesh_raycast.hip) and writes only the faces that see past the mesh in at least one of them, on either side: interior
shells go, exterior surface stays whether or not a camera saw it.  It needs no cameras; it comes after the clean-up and before
--drop-unseen.  Without the flag the file is what it was.

--mesh-largest K / --mesh-min-faces N keep the K largest connected components of the finished MESH, those of at least N faces
(mesh.keep_components, csrc/mesh_topology.hip; faces joined by their edges): the islands that --drop-unseen and
--drop-interior cut loose go, which the lattice options --keep-largest / --min-component cannot see.  --close-holes N then
caps every closed boundary loop of at most N edges with a fan round its centroid (mesh.close_holes): right for the small
cuts those options leave, wrong for large or bent holes, hence the limit.  --report-topology prints `topology: {JSON}` of the
mesh that is written (mesh.topology: components, boundary / non-manifold / inconsistent edges, Euler characteristic, genus,
loops).  --remesh RES [--remesh-offset D] then extracts the mesh again from its own signed distance field at RES lattice points
per axis, at the level D (mesh.remesh, csrc/mesh_sdf.hip): a closed, evenly tessellated surface in place of fans and slivers;
it needs a closed, consistently oriented mesh (--report-topology says) and drops the colours.  They come after all other
clean-up, in this order, and before --texture.  Without the flags every output is what
it was.

--report-error prints what the clean-up cost: the distance report of the finished mesh (after --smooth, --simplify and
--drop-unseen) against the mesh as first extracted (evaluate.mesh_distance_metrics, csrc/mesh_distance.hip: Chamfer and sampled
Hausdorff distance, precision / recall / F-score at half a, one and two lattice steps, normal consistency), as one line
`error report: {JSON}` in world units, with the largest lattice step under "lattice_step".  It changes no file; without the
flag the tool's output is what it was.

--texture N bakes a texture atlas of N texels along every face's leg (1..32) from the training views (mesh.bake_texture,
csrc/texture.hip) and writes Wavefront OBJ + MTL + PNG; --out must end in .obj.  It comes after all clean-up and after
--drop-unseen, so it textures the mesh that is written.  The images are renders of the field at the training cameras
(--texture-from render, the default) or the loader's images (--texture-from dataset); the cameras are those of --tsdf, else
--datadir / --factor.  Texels that no view sees are filled from the field (the head-on query of the vertex colours).  --out
*.obj without --texture writes the OBJ alone, with no texture coordinates.  Without the two flags every output is what it was.

--save-region PATH / --save-occupancy PATH voxelise the mesh that is written (mesh.voxelize, csrc/mesh_voxel.hip: the cells its
faces touch and the cells inside, by column parity with a majority of three axes) on the extraction box at --grid-cells cells
per axis, dilated --grid-dilate rounds, and save it as a region (Region.from_mesh: the masks of the object in every view, and
its carve) or as an occupancy grid (OccupancyGrid.from_mesh: a render with it shows the scene ONLY where the mesh is).  The
set cells, the dropped faces and the odd columns (the leak diagnostic) are printed.  Without the flags every output is what it
was.

--tsdf meshes what the renderer sees instead of thresholding sigma (mesh.fuse_depths): the disparity of every view (every
S-th with --view-step S) is rendered and fused into a truncated signed distance field whose zero level set is extracted
over the observed cells; --threshold is not used.  It needs the cameras, taken the way tools/prepare_depths.py takes them:
--fixture trains the scene-1 fixture, a checkpoint comes with --datadir / --factor.  --trunc: the truncation distance
(default: four times the largest lattice step).  Without --bound-min / --bound-max the box is the cameras' frustum box
(mesh.frustum_bounds).  Prints the observed share of the lattice and each stage's time.
"""
import argparse
import json
import os
import sys
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from mvip_nerf_amd import evaluate, mesh, ops, run                             # noqa: E402


def model_args(n_importance):
    """create_nerf / create_nerf_tcnn arguments of the reference's model (8x256 MLP, multires 10 / 4, view directions),
    world-space rays (no NDC), nothing reloaded from a directory: the checkpoint is loaded here."""
    return types.SimpleNamespace(
        multires=10, i_embed=0, use_viewdirs=True, multires_views=4, N_importance=n_importance, alpha_model_path=None,
        netdepth=8, netwidth=256, netdepth_fine=8, netwidth_fine=256, netchunk=65536, lrate=5e-4, basedir='.',
        expname='', ft_path=None, no_reload=True, perturb=0., N_samples=64, white_bkgd=False, raw_noise_std=0.,
        dataset_type='llff', no_ndc=True, lindisp=False, sigma_loss=False)


def load_model(path, model, device):
    ckpt = torch.load(path, map_location=device, weights_only=False)
    fine = ckpt.get('network_fine_state_dict')
    create = run.create_nerf if model == 'mlp' else run.create_nerf_tcnn
    _, kw, _, _, _ = create(model_args(64 if fine is not None else 0), device=device)
    kw['network_fn'].load_state_dict(run._strip_module_prefix(ckpt['network_fn_state_dict']))
    if fine is not None:
        kw['network_fine'].load_state_dict(run._strip_module_prefix(fine))
    return kw, int(ckpt.get('global_step', 0))


def _timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def clean_up(a, m, lo, hi, res):
    """--smooth, then --simplify, on the Mesh m extracted on the lattice `res` of the box [lo, hi]; (mesh, seconds)."""
    if not a.smooth and not a.simplify:
        return m, 0.0
    res3 = (res,) * 3 if np.isscalar(res) else tuple(res)
    lo32, hi32 = mesh._bounds(lo, hi)
    h = max(float((hi32[k] - lo32[k]) / np.float32(res3[k] - 1)) for k in range(3))

    def run():
        out = mesh.smooth(m, a.smooth) if a.smooth else m
        return mesh.simplify(out, a.simplify * h, a.simplify_placement) if a.simplify else out
    out, t = _timed(run)
    what = ' + '.join(([f'{a.smooth} Taubin iterations'] if a.smooth else [])
                      + ([f'clustering at {a.simplify:g} lattice steps ({a.simplify_placement})'] if a.simplify else []))
    print(f'{what}: {m.faces.shape[0]} triangles, {m.verts.shape[0]} vertices -> {out.faces.shape[0]} triangles, '
          f'{out.verts.shape[0]} vertices')
    return out, t


def report_error(a, first, m, lo, hi, res):
    """--report-error: the finished Mesh m against the Mesh `first` as extracted, printed as one JSON line."""
    if not a.report_error:
        return
    res3 = (res,) * 3 if np.isscalar(res) else tuple(res)
    lo32, hi32 = mesh._bounds(lo, hi)
    h = max(float((hi32[k] - lo32[k]) / np.float32(res3[k] - 1)) for k in range(3))
    if not m.faces.shape[0] or not first.faces.shape[0]:
        print('error report: null  (a mesh without faces)')
        return
    rep = evaluate.mesh_distance_metrics(m, first, samples=2, thresholds=(0.5 * h, h, 2.0 * h))
    rep['lattice_step'] = h
    print('error report: ' + json.dumps(rep))


def drop_interior(a, m):
    """--drop-interior on the finished Mesh m: (mesh, seconds)."""
    if not a.drop_interior:
        return m, 0.0
    out, t = _timed(lambda: mesh.drop_interior(m, directions=a.drop_interior))
    print(f'open in at least one of {a.drop_interior} directions: {m.faces.shape[0]} triangles, {m.verts.shape[0]} vertices '
          f'-> {out.faces.shape[0]} triangles, {out.verts.shape[0]} vertices  ({t * 1e3:.1f} ms)')
    return out, t


def drop_unseen(a, m, hwf, poses):
    """--drop-unseen on the finished Mesh m: (mesh, seconds)."""
    if not a.drop_unseen:
        return m, 0.0
    out, t = _timed(lambda: mesh.keep_faces(m, mesh.visible_faces(m, hwf, poses)))
    print(f'visible from {poses.shape[0]} views of {int(hwf[0])} x {int(hwf[1])}: {m.faces.shape[0]} triangles, {m.verts.shape[0]} vertices '
          f'-> {out.faces.shape[0]} triangles, {out.verts.shape[0]} vertices')
    return out, t


def mesh_topology_options(a, m):
    """--mesh-largest / --mesh-min-faces, --close-holes, --remesh, --report-topology on the finished Mesh m, in this order: (mesh,
    seconds)."""
    t = 0.0
    if a.mesh_largest is not None or a.mesh_min_faces is not None:
        out, dt = _timed(lambda: mesh.keep_components(m, largest=a.mesh_largest, min_faces=a.mesh_min_faces))
        print(f'mesh components kept: {m.faces.shape[0]} triangles, {m.verts.shape[0]} vertices -> {out.faces.shape[0]} triangles, '
              f'{out.verts.shape[0]} vertices  ({dt * 1e3:.1f} ms)')
        m, t = out, t + dt
    if a.close_holes:
        (out, capped, left), dt = _timed(lambda: mesh.close_holes(m, max_edges=a.close_holes))
        print(f'holes of at most {a.close_holes} edges: {capped} capped, {left} loops left open, {m.faces.shape[0]} -> '
              f'{out.faces.shape[0]} triangles  ({dt * 1e3:.1f} ms)')
        m, t = out, t + dt
    if a.remesh:
        out, dt = _timed(lambda: mesh.remesh(m, resolution=a.remesh, offset=a.remesh_offset))
        print(f'remeshed at {a.remesh} points per axis, offset {a.remesh_offset:g}: {m.faces.shape[0]} triangles, {m.verts.shape[0]} '
              f'vertices -> {out.faces.shape[0]} triangles, {out.verts.shape[0]} vertices, colours dropped  ({dt * 1e3:.1f} ms)')
        m, t = out, t + dt
    if a.report_topology:
        rep = mesh.topology(m)
        rep['per_component'] = rep['per_component'][:16]                     # the leading ones; `components` has the count
        print('topology: ' + json.dumps(rep))
    return m, t


def save_grids(a, m, lo, hi):
    """--save-region / --save-occupancy: the grids of the finished Mesh m on the box [lo, hi]."""
    if not a.save_region and not a.save_occupancy:
        return
    from mvip_nerf_amd.occupancy import OccupancyGrid
    from mvip_nerf_amd.region import Region
    (_, rep), t = _timed(lambda: mesh.voxelize(m, lo, hi, a.grid_cells))
    print(f'voxels at {a.grid_cells} cells per axis: {rep["count"]} set ({rep["volume"]:.6g} world units^3), {rep["dropped"]} faces dropped, '
          f'odd columns {rep["odd_columns"]}  ({t * 1e3:.1f} ms)')
    for path, cls in ((a.save_region, Region), (a.save_occupancy, OccupancyGrid)):
        if path:
            g = cls.from_mesh(m, lo, hi, cells=a.grid_cells, dilate=a.grid_dilate)
            g.save(path)
            print(f'{cls.NOUN}: {g.count()} of {g.n_cells} cells after {a.grid_dilate} rounds of dilation -> {path}')


def view_images(a, te, hwf, poses, near, far, dataset):
    """--texture: uint8 images [V, H, W, 3] of the cameras poses: renders of the field, or dataset() with --texture-from dataset."""
    if a.texture_from == 'dataset':
        im = torch.as_tensor(dataset()).to(poses.device)
        return im if im.dtype == torch.uint8 else (im.float() * 255.0 + 0.5).floor().clamp(0, 255).to(torch.uint8)
    H, W, focal = int(hwf[0]), int(hwf[1]), float(hwf[2])
    kw = dict(te, near=near, far=far)
    with torch.no_grad():
        rgb = torch.stack([run.render(H, W, focal, chunk=1 << 15, c2w=poses[n], **kw)[0].reshape(H, W, 3) for n in range(poses.shape[0])])
    return (rgb.float() * 255.0 + 0.5).floor().clamp(0, 255).to(torch.uint8)


def dataset_images(a):
    """--tsdf --texture-from dataset: the loader's images of the fused views."""
    if a.fixture:
        from tools import render_occupancy_ab as T
        return np.load(T.FIXTURE)['images'][::a.view_step]
    from mvip_nerf_amd.load_llff import load_llff_data
    return load_llff_data(a.datadir, factor=a.factor)[0][::a.view_step]


def write_mesh(a, m, te, hwf, poses, near, far, dataset):
    """Writes a.out: PLY, or OBJ (+ MTL + PNG with --texture).  (seconds of the bake, seconds of the write)."""
    if not a.out.endswith('.obj'):
        return 0.0, _timed(lambda: mesh.save_ply(a.out, m))[1]
    tex, t_tex = None, 0.0
    if a.texture:
        images, t_img = _timed(lambda: view_images(a, te, hwf, poses, near, far, dataset))
        tex, t_tex = _timed(lambda: mesh.bake_texture(m, hwf, poses, images, texels=a.texture, render_kwargs=te, network=a.network))
        print(f'texture from {poses.shape[0]} views of {int(hwf[0])} x {int(hwf[1])} ({a.texture_from}): {tuple(tex.image.shape[:2])} texels, '
              f'images {t_img * 1e3:.1f} ms, bake {t_tex * 1e3:.1f} ms')
    files, t_out = _timed(lambda: mesh.save_obj(a.out, m, tex))
    print('wrote ' + ', '.join(files))
    return t_tex, t_out


def main_tsdf(ap, a, res, dev):
    """--tsdf: render the views' disparities, fuse them, extract the zero level set over the observed cells."""
    from mvip_nerf_amd import prepare
    from tools import propagate_masks as P
    if a.fixture == bool(a.ckpt) or bool(a.ckpt) != bool(a.datadir) or a.view_step < 1:
        ap.error('--tsdf: either --fixture, or a checkpoint with --datadir; --view-step >= 1')
    if a.model != 'mlp':
        ap.error('--tsdf: the cameras are taken with the mlp model only')
    dataset = lambda: dataset_images(a)
    (te, hwf, poses, _, _, names, near, far, source), t_model = _timed(
        lambda: P.fixture_scene(dev, a.iters) if a.fixture else P.checkpoint_scene(dev, a.ckpt, a.datadir, a.factor))
    for net in (te['network_fn'], te.get('network_fine')):
        if net is not None:
            net.inference_precision = 1 if a.precision == 'split' else 0
    poses = poses[::a.view_step, :3, :4].contiguous().float()
    if (a.bound_min is None) != (a.bound_max is None):
        ap.error('--bound-min and --bound-max come together')
    lo, hi = (a.bound_min, a.bound_max) if a.bound_min is not None else mesh.frustum_bounds(poses, hwf, near, far)
    if (a.max_spread is not None and not a.max_spread >= 0) or (a.min_agree is not None and a.min_agree < 0) \
            or (a.max_violated is not None and a.max_violated < 0):
        ap.error('--max-spread, --min-agree and --max-violated must be >= 0')
    (disp, poses, keep, shares), t_render = _timed(lambda: mesh.filtered_disparities(
        te, hwf, poses, near, far, depth=a.tsdf_depth, max_spread=a.max_spread, min_agree=a.min_agree, max_violated=a.max_violated))
    lo32, hi32 = mesh._bounds(lo, hi)
    res3 = (res,) * 3 if np.isscalar(res) else tuple(res)
    trunc = a.trunc if a.trunc is not None else 4.0 * max(float((hi32[k] - lo32[k]) / np.float32(res3[k] - 1)) for k in range(3))
    (tsdf, count), t_fuse = _timed(lambda: ops.tsdf_fuse(disp, poses, hwf[2], lo32, hi32, res3, trunc, masks=keep))
    valid = count > 0
    g = torch.where(valid, 1.0 - tsdf, torch.zeros((), device=dev))
    print(f'{source}: {poses.shape[0]} views of {hwf[0]} x {hwf[1]}, lattice {tuple(tsdf.shape)} in {[round(float(v), 4) for v in lo32]} .. '
          f'{[round(float(v), 4) for v in hi32]}, trunc {trunc:.4g}')
    if a.tsdf_depth != 'expected' or shares:
        print(f'depth maps: {a.tsdf_depth}' + ''.join(f', {k} filter masks {v:.4f} of the pixels' for k, v in shares.items()))
    print(f'observed share of the lattice {float(valid.float().mean()):.4f}  (inside: {float((valid & (tsdf <= 0)).float().mean()):.4f})')
    t_cc = 0.0
    if a.keep_largest is not None or a.min_component is not None:
        n_before = int(ops.grid_components(ops.grid_pack(g, 1.0), g.shape)[1].shape[0])
        g, t_cc = _timed(lambda: mesh.remove_floaters(g, 1.0, a.keep_largest, a.min_component))
        n_after = int(ops.grid_components(ops.grid_pack(g, 1.0), g.shape)[1].shape[0])
        print(f'components of the inside points: {n_before} -> {n_after} kept')
    (verts, faces, normals), t_mc = _timed(lambda: mesh.marching_cubes(g, 1.0, lo32, hi32, valid=valid))
    colors, t_col = (None, 0.0) if a.no_colors else _timed(lambda: mesh.vertex_colors(te, verts, normals, a.network))
    first = mesh.Mesh(verts, faces, normals, colors)
    m, t_clean = clean_up(a, first, lo32, hi32, res)
    m, _ = drop_interior(a, m)
    m, t_seen = drop_unseen(a, m, hwf, poses)
    m, _ = mesh_topology_options(a, m)
    report_error(a, first, m, lo32, hi32, res)
    save_grids(a, m, lo32, hi32)
    t_tex, t_ply = write_mesh(a, m, te, hwf, poses, near, far, dataset)
    print(f'tsdf zero level set: {m.verts.shape[0]} vertices, {m.faces.shape[0]} triangles -> {a.out}')
    print(f'time  model {t_model * 1e3:.1f} ms  render {t_render * 1e3:.1f} ms  fusion {t_fuse * 1e3:.1f} ms  components {t_cc * 1e3:.1f} ms  '
          f'marching cubes {t_mc * 1e3:.1f} ms  colours {t_col * 1e3:.1f} ms  clean-up {t_clean * 1e3:.1f} ms  '
          + (f'visibility {t_seen * 1e3:.1f} ms  ' if a.drop_unseen else '') + (f'texture {t_tex * 1e3:.1f} ms  ' if a.texture else '')
          + f'write {t_ply * 1e3:.1f} ms')
    return 0


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('ckpt', nargs='?')
    ap.add_argument('--out', required=True)
    ap.add_argument('--model', choices=('mlp', 'tcnn'), default='mlp')
    ap.add_argument('--bound-min', type=float, nargs=3, default=None, help='default -1 -1 -1; with --tsdf the frustum box')
    ap.add_argument('--bound-max', type=float, nargs=3, default=None, help='default 1 1 1; with --tsdf the frustum box')
    ap.add_argument('--resolution', type=int, nargs='+', default=[256], help='one count, or three')
    ap.add_argument('--threshold', type=float, default=10.0)
    ap.add_argument('--network', choices=('fine', 'coarse'), default='fine')
    ap.add_argument('--precision', choices=('fp32', 'split'), default='fp32', help='MLP query precision (mlp model)')
    ap.add_argument('--no-colors', action='store_true')
    ap.add_argument('--keep-largest', type=int, default=None, metavar='K', help='keep the K largest components')
    ap.add_argument('--min-component', type=int, default=None, metavar='N', help='drop components below N lattice points')
    ap.add_argument('--smooth', type=int, default=0, metavar='ITERS', help='Taubin smoothing iterations (0: off)')
    ap.add_argument('--simplify', type=float, default=0.0, metavar='STEPS',
                    help='cluster the vertices in cells of STEPS times the largest lattice step (0: off)')
    ap.add_argument('--simplify-placement', choices=('quadric', 'mean'), default='quadric')
    ap.add_argument('--drop-interior', type=int, default=0, metavar='K',
                    help='write only the faces that see past the mesh in at least one of K Fibonacci directions (0: off)')
    ap.add_argument('--drop-unseen', action='store_true',
                    help='write only the faces some training view sees (cameras: those of --tsdf, else --datadir / --factor)')
    ap.add_argument('--texture', type=int, default=0, metavar='N',
                    help='bake a texture atlas of N texels per face leg from the training views and write OBJ + MTL + PNG (0: off)')
    ap.add_argument('--texture-from', choices=('render', 'dataset'), default='render',
                    help='--texture: the images are renders of the field at the training cameras, or the dataset\'s')
    ap.add_argument('--mesh-largest', type=int, default=None, metavar='K', help='keep the K largest components of the finished mesh')
    ap.add_argument('--mesh-min-faces', type=int, default=None, metavar='N', help='drop mesh components below N faces')
    ap.add_argument('--close-holes', type=int, default=0, metavar='N',
                    help='cap the closed boundary loops of at most N edges with a centroid fan (0: off)')
    ap.add_argument('--remesh', type=int, default=0, metavar='RES',
                    help='extract the mesh again from its own signed distance field at RES lattice points per axis (0: off)')
    ap.add_argument('--remesh-offset', type=float, default=0.0, metavar='D', help='--remesh: the level, > 0 grows the shape')
    ap.add_argument('--report-topology', action='store_true', help='print the topology report of the mesh that is written')
    ap.add_argument('--report-error', action='store_true',
                    help='print the distance report of the finished mesh against the mesh as first extracted')
    ap.add_argument('--save-region', metavar='PATH', help='save the written mesh as a region (.npz)')
    ap.add_argument('--save-occupancy', metavar='PATH', help='save the written mesh as an occupancy grid (.npz)')
    ap.add_argument('--grid-cells', type=int, default=128, metavar='N', help='cells per axis of the saved grids')
    ap.add_argument('--grid-dilate', type=int, default=1, metavar='R', help='dilation rounds of the saved grids')
    ap.add_argument('--tsdf', action='store_true', help='fuse rendered depth maps instead of thresholding sigma')
    ap.add_argument('--fixture', action='store_true', help='--tsdf: train the scene-1 fixture and use its cameras')
    ap.add_argument('--iters', type=int, default=1500, help='training iterations of --fixture')
    ap.add_argument('--datadir', help='--tsdf with a checkpoint: the scene whose cameras are rendered; --drop-unseen: its cameras')
    ap.add_argument('--factor', type=int, default=4)
    ap.add_argument('--trunc', type=float, default=None, help='--tsdf: truncation distance (default: 4 lattice steps)')
    ap.add_argument('--view-step', type=int, default=1, metavar='S', help='--tsdf: fuse every S-th view')
    ap.add_argument('--tsdf-depth', choices=('expected', 'median'), default='expected',
                    help='--tsdf: fuse the expected ray depth (default) or the median termination depth')
    ap.add_argument('--max-spread', type=float, default=None, metavar='R',
                    help='--tsdf: drop the pixels whose ray has (z(0.84) - z(0.16)) / z(0.5) > R (default: off; tools/depth_quality.py '
                         'suggests a value)')
    ap.add_argument('--min-agree', type=int, default=None, metavar='K', help='--tsdf: drop the pixels fewer than K other views confirm')
    ap.add_argument('--max-violated', type=int, default=None, metavar='K',
                    help='--tsdf: drop the pixels more than K other views see through')
    a = ap.parse_args(argv)
    if a.smooth < 0 or not a.simplify >= 0:
        ap.error('--smooth and --simplify must be >= 0')
    if not 0 <= a.drop_interior <= 255:
        ap.error('--drop-interior: 1..255 directions')
    if (a.mesh_largest is not None and a.mesh_largest < 1) or (a.mesh_min_faces is not None and a.mesh_min_faces < 1):
        ap.error('--mesh-largest and --mesh-min-faces must be >= 1')
    if a.remesh != 0 and not 8 <= a.remesh <= mesh.MAX_POINTS_PER_AXIS:
        ap.error(f'--remesh: 8..{mesh.MAX_POINTS_PER_AXIS} lattice points per axis')
    if a.remesh_offset != 0.0 and not a.remesh:
        ap.error('--remesh-offset belongs to --remesh')
    if a.close_holes != 0 and a.close_holes < 3:
        ap.error('--close-holes: at least 3 edges (0: off)')
    if not 0 <= a.texture <= 32 or (a.texture and not a.out.endswith('.obj')):
        ap.error('--texture: 1..32 texels, and --out must end in .obj')
    if not 1 <= a.grid_cells <= 512 or not 0 <= a.grid_dilate <= 512:
        ap.error('--grid-cells: 1..512, --grid-dilate: 0..512')
    res = a.resolution[0] if len(a.resolution) == 1 else tuple(a.resolution)
    dev = torch.device('cuda', 0)
    if a.tsdf:
        return main_tsdf(ap, a, res, dev)
    if a.fixture or a.ckpt is None or bool(a.datadir) != (a.drop_unseen or bool(a.texture)):
        ap.error('a checkpoint is required; --fixture belongs to --tsdf, --datadir to --tsdf, --drop-unseen or --texture (which need it)')
    a.bound_min = (-1.0, -1.0, -1.0) if a.bound_min is None else a.bound_min
    a.bound_max = (1.0, 1.0, 1.0) if a.bound_max is None else a.bound_max
    kw, step = load_model(a.ckpt, a.model, dev)
    if a.model == 'mlp':
        for net in (kw['network_fn'], kw['network_fine']):
            if net is not None:
                net.inference_precision = 1 if a.precision == 'split' else 0

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return out, time.perf_counter() - t0

    grid, t_grid = timed(lambda: mesh.density_grid(kw, a.bound_min, a.bound_max, res, a.network))
    q = np.percentile(grid.float().cpu().numpy(), [1, 5, 25, 50, 75, 95, 99])
    print(f'checkpoint {a.ckpt} (step {step}, model {a.model}, {a.network} network), grid {tuple(grid.shape)}')
    print('sigma percentiles  ' + '  '.join(f'p{p}={v:.4g}' for p, v in zip((1, 5, 25, 50, 75, 95, 99), q)))
    t_cc = 0.0
    if a.keep_largest is not None or a.min_component is not None:
        n_before = int(ops.grid_components(ops.grid_pack(grid, a.threshold), grid.shape)[1].shape[0])
        grid, t_cc = timed(lambda: mesh.remove_floaters(grid, a.threshold, a.keep_largest, a.min_component))
        n_after = int(ops.grid_components(ops.grid_pack(grid, a.threshold), grid.shape)[1].shape[0])
        print(f'components of the inside points: {n_before} -> {n_after} kept')
    (verts, faces, normals), t_mc = timed(lambda: mesh.marching_cubes(grid, a.threshold, a.bound_min, a.bound_max))
    colors, t_col = (None, 0.0) if a.no_colors else timed(lambda: mesh.vertex_colors(kw, verts, normals, a.network))
    first = mesh.Mesh(verts, faces, normals, colors)
    m, t_clean = clean_up(a, first, a.bound_min, a.bound_max, res)
    m, _ = drop_interior(a, m)
    t_seen, hwf, cam_poses, near, far, loaded = 0.0, None, None, None, None, None
    if a.drop_unseen or a.texture:
        from mvip_nerf_amd.load_llff import load_llff_data
        loaded = load_llff_data(a.datadir, factor=a.factor)
        cams, bds = loaded[1], loaded[2]
        hwf, cam_poses = tuple(float(v) for v in cams[0, :3, -1]), torch.from_numpy(cams[:, :3, :4].copy()).to(dev)
        near, far = float(bds.min() * .9), float(bds.max() * 1.)
    if a.drop_unseen:
        m, t_seen = drop_unseen(a, m, hwf, cam_poses)
    m, _ = mesh_topology_options(a, m)
    report_error(a, first, m, a.bound_min, a.bound_max, res)
    save_grids(a, m, a.bound_min, a.bound_max)
    t_tex, t_ply = write_mesh(a, m, kw, hwf, cam_poses, near, far, lambda: loaded[0])
    print(f'threshold {a.threshold}: {m.verts.shape[0]} vertices, {m.faces.shape[0]} triangles -> {a.out}')
    print(f'time  density grid {t_grid * 1e3:.1f} ms  components {t_cc * 1e3:.1f} ms  marching cubes {t_mc * 1e3:.1f} ms  colours {t_col * 1e3:.1f} ms  '
          f'clean-up {t_clean * 1e3:.1f} ms  ' + (f'visibility {t_seen * 1e3:.1f} ms  ' if a.drop_unseen else '')
          + (f'texture {t_tex * 1e3:.1f} ms  ' if a.texture else '') + f'write {t_ply * 1e3:.1f} ms')
    return 0


if __name__ == '__main__':
    sys.exit(main())
