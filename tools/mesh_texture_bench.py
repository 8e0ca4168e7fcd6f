"""Mesh texturing timings (profiles/mesh_texture.json): csrc/texture.hip on the three meshes of tools/mesh_raster_bench.py (the
analytic sphere and the 4-period gyroid at 256^3, and the gyroid clustered at 8 lattice steps), 30 views of 378 x 504 on the same
orbit, at 4 and 8 texels per face leg where the atlas fits into 16,384 texels a side.  The images are seeded noise (the kernel's
work does not depend on their content), the disparities the rasteriser's own.  HIP-event times, the median of 5 windows after a
warm-up, on preallocated buffers: the atlas bake with texels mapped to lanes in texture row-major order and in block-major order
(the A/B behind ops.mesh_bake_atlas's default), the bake of the vertices (mesh_bake_points), the textured resolve next to the
rasteriser's colour resolve.  From the outputs: the (texel, view) pairs per second (owned texels x views over the bake time) and
the pairs that contribute.  A record, not a gate.

Bytes, from the shapes: a bake writes 11 bytes per texel (3 rgb, 4 wsum, 4 best); per owned texel it reads 12 bytes of indices
and 36 of positions (cached: a block's texels share two faces), per (texel, view) pair 48 bytes of pose (wave-uniform), and per
pair that passes the projection and facing tests 16 bytes of disparity and, when visible, 12 of image.

--scene1 (profiles/mesh_texture_scene1.json): the scene-1 fixture field of --iters training iterations; every tenth view is held
out, the TSDF mesh is fused from the field's disparities of the other views and textured from the DATASET's images of those
views; evaluate.mesh_image_metrics on the held-out views against the dataset's images there, for the field-queried vertex
colours (what the exporter wrote so far), mesh.colors_from_views, and textures at 4 and 8 texels, on the TSDF mesh and on its
smoothed (5 Taubin iterations) and clustered (4 lattice steps) form.

  python tools/mesh_texture_bench.py [--out profile_out/mesh_texture.json] [--size 256] [--views 30] [--commit HASH]
  python tools/mesh_texture_bench.py --scene1 [--iters 1500] [--resolution 256] [--out profile_out/mesh_texture_scene1.json]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from mvip_nerf_amd import mesh, ops                                  # noqa: E402
from mvip_nerf_amd._lib import ptr, stream, call                     # noqa: E402
from tools.mesh_bench import event_ms, gyroid                        # noqa: E402
from tools.mesh_ops_bench import sphere, LO, HI                      # noqa: E402
from tools.mesh_raster_bench import orbit, H, W, FOCAL, NEAR         # noqa: E402

I32, I64, U8 = torch.int32, torch.int64, torch.uint8
TOL = 0.05


def row(name, v, f, poses, images, texels):
    dev = v.device
    Nv, F, V = int(v.shape[0]), int(f.shape[0]), int(poses.shape[0])
    try:
        Ht, Wt, _, _, S = ops.texture_layout(F, texels)
    except ValueError as e:
        return {'mesh': name, 'triangles': F, 'texels': texels, 'skipped': str(e)}
    disp, face, _ = ops.mesh_rasterize(v, f, poses, H, W, FOCAL)
    normals = ops.mesh_vertex_normals(v, f)
    col = torch.randint(0, 256, (Nv, 3), device=dev, dtype=U8, generator=torch.Generator(device=dev).manual_seed(1))
    rgb = torch.empty((Ht, Wt, 3), device=dev, dtype=U8)
    wsum = torch.empty((Ht, Wt), device=dev)
    best = torch.empty((Ht, Wt), device=dev, dtype=I32)
    prgb = torch.empty((Nv, 3), device=dev, dtype=U8)
    pwsum = torch.empty(Nv, device=dev)
    pbest = torch.empty(Nv, device=dev, dtype=I32)
    flag = torch.empty(1, device=dev, dtype=I32)
    out = torch.empty((V, H, W, 3), device=dev, dtype=U8)
    keys = torch.empty((V, H, W), device=dev, dtype=I64)
    d2 = torch.empty((V, H, W), device=dev)
    f2 = torch.empty((V, H, W), device=dev, dtype=I32)
    none = ptr(None)
    views = (ptr(images, U8), ptr(disp), none, ptr(poses), V, H, W, FOCAL, NEAR, TOL, 1, 0)

    def atlas(order):
        call('mvip_texture_bake_atlas', ptr(v), ptr(f, I32), Nv, F, texels, order, *views, ptr(rgb, U8), ptr(wsum), ptr(best, I32),
             ptr(flag, I32), stream())

    def points():
        call('mvip_texture_bake_points', ptr(v), ptr(normals), Nv, *views, ptr(prgb, U8), ptr(pwsum), ptr(pbest, I32), stream())

    def resolve():
        call('mvip_texture_resolve', ptr(face, I32), ptr(v), ptr(f, I32), Nv, F, ptr(rgb, U8), texels, ptr(poses), V, H, W, FOCAL, NEAR,
             ptr(out, U8), stream())

    def colour_resolve():
        call('mvip_raster_resolve', ptr(keys, I64), ptr(v), ptr(f, I32), ptr(col, U8), Nv, F, ptr(poses), V, H, W, FOCAL, NEAR, ptr(d2),
             ptr(f2, I32), ptr(out, U8), stream())

    call('mvip_raster_fragments', ptr(v), ptr(f, I32), Nv, F, ptr(poses), V, H, W, FOCAL, NEAR, 0, ptr(keys, I64), ptr(flag, I32), none, stream())
    t_row, reps_row = event_ms(lambda: atlas(0), warmup=1)
    t_blk, reps_blk = event_ms(lambda: atlas(1), warmup=1)
    assert int(flag.cpu()) == 0
    t_pts, _ = event_ms(points, warmup=1)
    t_res, _ = event_ms(resolve, warmup=1)
    t_col, _ = event_ms(colour_resolve, warmup=1)
    owned = int(mesh._owned_texels(F, texels, dev).sum())
    seen = int((best >= 0).sum())
    pairs = owned * V
    t_best = min(t_row, t_blk)
    return {'mesh': name, 'vertices': Nv, 'triangles': F, 'views': V, 'image': [H, W], 'focal': FOCAL, 'texels': texels,
            'atlas': [Ht, Wt], 'atlas_texels': Ht * Wt, 'owned_texels': owned, 'seen_texels': seen,
            'unseen_share_of_owned': round(1 - seen / max(owned, 1), 4),
            'ms_bake_atlas_row_major': round(t_row, 4), 'ms_bake_atlas_row_major_reps': [round(t, 4) for t in reps_row],
            'ms_bake_atlas_block_major': round(t_blk, 4), 'ms_bake_atlas_block_major_reps': [round(t, 4) for t in reps_blk],
            'texel_view_pairs': pairs, 'texel_view_pairs_per_second': round(pairs / (t_best * 1e-3)),
            'sum_of_weights': round(float(wsum.double().sum()), 1),
            'bytes_written_by_a_bake': 11 * Ht * Wt, 'bytes_of_images_and_disparities': V * H * W * 7,
            'ms_bake_points_at_the_vertices': round(t_pts, 4), 'vertices_seen': int((pbest >= 0).sum()),
            'ms_textured_resolve': round(t_res, 4), 'ms_colour_resolve_of_the_rasteriser': round(t_col, 4)}


def contributing_pairs(v, f, poses, images, texels):
    """the (texel, view) pairs that contribute, counted exactly: one bake per view alone."""
    disp = ops.mesh_rasterize(v, f, poses, H, W, FOCAL)[0]
    total = 0
    for k in range(poses.shape[0]):
        best = ops.mesh_bake_atlas(v, f, texels, images[k:k + 1], disp[k:k + 1], poses[k:k + 1], FOCAL)[2]
        total += int((best >= 0).sum())
    return total


def scene1(a, dev):
    import numpy as np
    from mvip_nerf_amd import evaluate, prepare
    from tools import render_occupancy_ab as T
    scene = T.train_scene1(dev, a.iters)
    te, near, far = scene['te'], scene['near'], scene['far']
    hwf = (scene['H'], scene['W'], scene['focal'])
    poses = scene['poses'][:, :3, :4].contiguous().float()
    images = scene['images']
    held = list(range(0, poses.shape[0], 10))
    rest = [i for i in range(poses.shape[0]) if i not in held]
    lo, hi = mesh._bounds(*mesh.frustum_bounds(poses, hwf, near, far))
    h = max(float((hi[k] - lo[k]) / np.float32(a.resolution - 1)) for k in range(3))
    disp = prepare.render_disparities(te, hwf, poses[rest], near, far)
    m = mesh.fuse_depths(disp, poses[rest], float(hwf[2]), lo, hi, a.resolution)
    m = mesh.Mesh(m.verts, m.faces, m.normals, mesh.vertex_colors(te, m.verts, m.normals))
    rows = []
    for stage, mm in (('TSDF mesh', m), ('TSDF mesh, 5 Taubin + clustered at 4 steps', mesh.simplify(mesh.smooth(m, 5), 4.0 * h))):
        def add(colouring, texture, msh, **extra):
            rep = evaluate.mesh_image_metrics(msh, texture, hwf, poses[held], images[held])
            r = dict({'stage': stage, 'triangles': int(msh.faces.shape[0]), 'vertices': int(msh.verts.shape[0]), 'colouring': colouring,
                      'coverage': rep['mean']['coverage'], 'psnr': rep['mean']['psnr'], 'ssim': rep['mean']['ssim'],
                      'psnr_per_view': rep['per_view']['psnr']}, **extra)
            rows.append(r)
            print(json.dumps(r), flush=True)
        add('vertex colours queried from the field', None, mm)
        cm = mesh.colors_from_views(mm, hwf, poses[rest], images[rest])
        add('vertex colours baked from the views (colors_from_views)', None, cm)
        for texels in (4, 8):
            owned = int(mesh._owned_texels(int(mm.faces.shape[0]), texels, dev).sum())
            for fill in (False, True):
                tex = mesh.bake_texture(mm, hwf, poses[rest], images[rest], texels=texels, render_kwargs=te if fill else None)
                add(f'texture at {texels} texels' + (', unseen texels filled from the field' if fill else ', unseen texels 0'), tex, mm,
                    atlas=[int(x) for x in tex.image.shape[:2]], unseen_share_of_owned_texels=round(1 - int(tex.seen.sum()) / max(owned, 1), 4))
    out = {'commit': a.commit, 'device': torch.cuda.get_device_name(0), 'fixture': 'tests/golden/scene1_small.npz', 'iterations': a.iters,
           'held_out_views': held, 'baked_from_views': len(rest), 'image': [int(hwf[0]), int(hwf[1])], 'resolution': a.resolution,
           'images': 'the dataset\'s', 'rows': rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fh:
        json.dump(out, fh, indent=1)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--views', type=int, default=30)
    ap.add_argument('--commit', default='')
    ap.add_argument('--scene1', action='store_true', help='the held-out image metrics on the scene-1 fixture field instead')
    ap.add_argument('--iters', type=int, default=1500, help='--scene1: training iterations')
    ap.add_argument('--resolution', type=int, default=256, help='--scene1: lattice points per axis of the TSDF')
    a = ap.parse_args()
    dev = torch.device('cuda', 0)
    a.out = a.out or os.path.join(ROOT, 'profile_out', 'mesh_texture_scene1.json' if a.scene1 else 'mesh_texture.json')
    if a.scene1:
        return scene1(a, dev)
    n = a.size
    poses = orbit(a.views, dev)
    images = torch.randint(0, 256, (a.views, H, W, 3), device=dev, dtype=U8, generator=torch.Generator(device=dev).manual_seed(2))
    meshes = []
    v, f, _ = mesh.marching_cubes(sphere(n, dev), 1.0, LO, HI)
    meshes.append(('analytic sphere, radius 0.6, iso 1', v, f))
    v, f, _ = mesh.marching_cubes(gyroid(n, dev), 1.5, LO, HI)
    meshes.append(('gyroid, 4 periods, iso 1.5', v, f))
    cv, cf, _, _ = ops.mesh_cluster(v, f, None, None, 8 * 2.0 / (n - 1), 'quadric')
    meshes.append(('the gyroid clustered at 8 lattice steps', cv, cf))
    rows = []
    for name, mv, mf in meshes:
        for texels in (4, 8):
            r = row(name, mv, mf, poses, images, texels)
            if 'skipped' not in r:
                r['contributing_pairs'] = contributing_pairs(mv, mf, poses, images, texels)
                r['contributing_share_of_pairs'] = round(r['contributing_pairs'] / max(r['texel_view_pairs'], 1), 4)
            rows.append(r)
            print(json.dumps(r), flush=True)
    out = {'commit': a.commit, 'device': torch.cuda.get_device_name(0), 'tol': TOL, 'cull': 'back', 'mode': 'blend', 'rows': rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fh:
        json.dump(out, fh, indent=1)
    return 0


if __name__ == '__main__':
    sys.exit(main())
