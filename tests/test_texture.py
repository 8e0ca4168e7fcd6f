"""The mesh texturing on the GPU (csrc/texture.hip; ops.mesh_bake_points / mesh_bake_atlas / mesh_texture_resolve) against its
restatement tests/texture_numpy.py: the bits of rgb, wsum and best must be EQUAL EVERYWHERE -- the definition is fp64 and integers,
there is no tolerance and nothing is excluded -- and a repetition must be bit-equal.  Then mesh.bake_texture / colors_from_views /
render_textured, evaluate.mesh_image_metrics, the argument checks of ops and of the C ABI."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_ops_numpy as R                               # noqa: E402
import raster_numpy as N                                 # noqa: E402
import test_raster as TR                                 # noqa: E402  (the sphere, its poses and the large-triangle case)
import test_texture_cpu as C                             # noqa: E402  (the two-quad occlusion scene)
import texture_numpy as T                                # noqa: E402
import warp_numpy as Wn                                  # noqa: E402
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mvip_nerf_amd import _lib, evaluate, mesh, ops      # noqa: E402

pytestmark = pytest.mark.gpu

H, W, FOCAL = TR.H, TR.W, TR.FOCAL
IDENTITY = Wn.pose()
_cache = {}


def dev(a, cuda):
    return torch.from_numpy(np.array(a, order='C')).to(cuda)


def sphere_views():
    """the sphere, its three poses (one inside the sphere), the restatement's disparities and face maps, seeded images and masks."""
    if 'views' not in _cache:
        v, f, col = TR.sphere()
        poses = TR.sphere_poses()
        disp, fmap, _ = TR.reference('sphere', v, f, poses, 'none', None)
        rs = np.random.RandomState(17)
        images = rs.randint(0, 256, (3, H, W, 3)).astype(np.uint8)
        masks = rs.uniform(size=(3, H, W)) > 0.1
        for a in (images, masks):
            a.setflags(write=False)
        _cache['views'] = (v, f, poses, disp, fmap, images, masks)
    return _cache['views']


def assert_bits(got, want, what):
    rgb, wsum, best = (t.cpu().numpy() for t in got)
    assert rgb.dtype == np.uint8 and wsum.dtype == np.float32 and best.dtype == np.int32
    assert rgb.shape == want[0].shape and wsum.shape == want[1].shape and best.shape == want[2].shape
    nc = int((rgb != want[0]).any(-1).sum())
    nw = int((wsum.view(np.uint32) != want[1].view(np.uint32)).sum())
    nb = int((best != want[2]).sum())
    print(f'{what}: points that differ from the restatement: rgb {nc}, wsum {nw}, best {nb} of {best.size}; seen {int((want[2] >= 0).sum())}')
    assert nc == 0 and nw == 0 and nb == 0


def gpu_atlas(cuda, v, f, n, images, disp, poses, focal=FOCAL, masks=None, **kw):
    return ops.mesh_bake_atlas(dev(np.asarray(v, np.float32), cuda), dev(np.asarray(f, np.int32).reshape(-1, 3), cuda), n, dev(images, cuda),
                               dev(disp, cuda), dev(np.asarray(poses, np.float32).reshape(-1, 3, 4), cuda), focal,
                               masks=None if masks is None else dev(masks, cuda), **kw)


def gpu_points(cuda, p, nrm, images, disp, poses, focal=FOCAL, masks=None, **kw):
    return ops.mesh_bake_points(dev(np.asarray(p, np.float32).reshape(-1, 3), cuda), dev(np.asarray(nrm, np.float32).reshape(-1, 3), cuda),
                                dev(images, cuda), dev(disp, cuda), dev(np.asarray(poses, np.float32).reshape(-1, 3, 4), cuda), focal,
                                masks=None if masks is None else dev(masks, cuda), **kw)


@pytest.mark.parametrize('masked', [False, True])
@pytest.mark.parametrize('mode', T.MODES)
@pytest.mark.parametrize('cull', T.CULLS)
def test_sphere_atlas_equals_the_restatement(cull, mode, masked, cuda):
    v, f, poses, disp, _, images, masks = sphere_views()
    assert len(f) == 1772 and T.layout(len(f), 3)['Wt'] * T.layout(len(f), 3)['Ht'] > 1024
    m = masks if masked else None
    want = T.bake_atlas(v, f, 3, images, disp, poses, FOCAL, cull=cull, mode=mode, masks=m, details=True)
    per_view = [int((want[3][k] > 0).sum()) for k in range(3)]
    assert per_view[0] > 500 and per_view[1] > 500 and (per_view[2] > 500) == (cull == 'none')     # the third camera is inside
    got = gpu_atlas(cuda, v, f, 3, images, disp, poses, cull=cull, mode=mode, masks=m)
    assert_bits(got, want[:3], f'sphere atlas at 3 texels, cull {cull}, mode {mode}, masks {masked}; contributing pairs {per_view}')
    for order in ops.TEXTURE_ORDERS:                        # a repetition, and the other lane mapping
        again = gpu_atlas(cuda, v, f, 3, images, disp, poses, cull=cull, mode=mode, masks=m, order=order)
        for a, b in zip(got, again):
            assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))


@pytest.mark.parametrize('F,n', [(7, 1), (7, 32), (1, 8)])
def test_few_faces_smallest_and_largest_texel_counts(F, n, cuda):
    v, f, poses, disp, fmap, images, _ = sphere_views()
    pick = np.unique(fmap[0][fmap[0] >= 0])[100:100 + F]    # faces that view 0 sees
    fv, ff, _, _ = N.keep_faces(v, f, np.isin(np.arange(len(f)), pick))
    d = disp                                                # the whole sphere's: no footprint lies wholly on a lone face of a pixel's size
    want = T.bake_atlas(fv, ff, n, images, d, poses, FOCAL)
    owner = T.owner_map(F, n)[0]
    assert (want[2] >= 0).sum() > 0 and (want[0][owner < 0] == 0).all() and (want[2][owner < 0] == -1).all()
    assert F % 2 == 0 or (owner < 0).sum() >= (n + 3) * (n + 2) // 2                  # odd F: the unowned half stays 0
    assert_bits(gpu_atlas(cuda, fv, ff, n, images, d, poses), want, f'{F} faces at {n} texels')
    assert_bits(gpu_atlas(cuda, fv, ff, n, images, d, poses, order='block'), want, f'{F} faces at {n} texels, block-major')


def test_occlusion_scene(cuda):
    v, f, poses, images, disp, _ = C.occlusion_scene()
    for n in (16, 5):
        for mode in T.MODES:
            want = T.bake_atlas(v, f, n, images, disp, poses, FOCAL, mode=mode)
            assert (want[2] == 1).sum() > 0 and (want[2] == 0).sum() > 10 and (want[2] == -1).sum() > 10
            assert_bits(gpu_atlas(cuda, v, f, n, images, disp, poses, mode=mode), want, f'two quads at {n} texels, mode {mode}')


def test_points_entry(cuda):
    v, f, poses, disp, _, images, masks = sphere_views()
    rs = np.random.RandomState(23)
    idx = rs.randint(0, len(v), 1000)
    p = (v[idx] + rs.normal(0, 2e-3, (1000, 3))).astype(np.float32)       # on and just off the surface
    nrm = (v[idx] * rs.uniform(0.5, 2.0, (1000, 1))).astype(np.float32)  # outward, not unit length
    for cull, mode, m in (('back', 'blend', None), ('none', 'best', masks), ('none', 'blend', None)):
        want = T.bake_points(p, nrm, images, disp, poses, FOCAL, cull=cull, mode=mode, masks=m)
        assert 100 < (want[2] >= 0).sum() < 1000
        got = gpu_points(cuda, p, nrm, images, disp, poses, cull=cull, mode=mode, masks=m)
        assert_bits(got, want, f'1000 points, cull {cull}, mode {mode}')
        again = gpu_points(cuda, p, nrm, images, disp, poses, cull=cull, mode=mode, masks=m)
        for a, b in zip(got, again):
            assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    e3 = np.zeros((0, 3), np.float32)
    rgb, wsum, best = gpu_points(cuda, e3, e3, images, disp, poses)                                  # N = 0
    assert rgb.shape == (0, 3) and wsum.shape == (0,) and best.shape == (0,)
    none = (np.zeros((0, H, W, 3), np.uint8), np.zeros((0, H, W), np.float32), np.zeros((0, 3, 4), np.float32))
    rgb, wsum, best = gpu_points(cuda, p, nrm, *none)                                               # V = 0
    assert torch.all(rgb == 0) and torch.all(wsum == 0) and torch.all(best == -1) and best.shape == (1000,)
    rgb, wsum, best = gpu_atlas(cuda, v, f, 3, *none)
    assert torch.all(rgb == 0) and torch.all(wsum == 0) and torch.all(best == -1) and best.shape == T.owner_map(len(f), 3)[0].shape
    rgb, wsum, best = gpu_atlas(cuda, v, np.zeros((0, 3), np.int32), 3, images, disp, poses)        # F = 0
    assert rgb.shape == (0, 0, 3) and wsum.shape == (0, 0) and best.shape == (0, 0)
    assert mesh.atlas_layout(0, 3)[0] == (0, 0, 3)


def test_borders_bad_points_and_bad_vertices(cuda):
    focal = 64.0                                            # the exact projections of tests/test_texture_cpu.py
    images = np.random.RandomState(3).randint(0, 256, (1, H, W, 3)).astype(np.uint8)
    disp = np.full((1, H, W), 0.5, np.float32)
    up = np.nextafter(np.float32(0.96875), np.float32(2))
    pts = np.array([[0.96875, 0.125, -2], [up, 0.125, -2], [0.25, 0.75, -2], [0.25, np.nextafter(np.float32(0.75), np.float32(2)), -2],
                    [-1.0, -0.71875, -2], [0.25, 0.125, -2], [0, 0, 2], [np.nan, 0, -2], [0, np.inf, -2], [0.25, 0.125, -2],
                    [0.25, 0.125, -2], [0.25, 0.125, -2]], np.float32)
    nrm = np.tile(np.array([[0, 0, 1]], np.float32), (len(pts), 1))
    nrm[9], nrm[10], nrm[11] = (0, 0, 0), (np.nan, 0, 1), (0, np.inf, 1)
    want = T.bake_points(pts, nrm, images, disp, IDENTITY[None], focal)
    assert want[2].tolist() == [0, -1, 0, -1, 0, 0, -1, -1, -1, -1, -1, -1]
    assert_bits(gpu_points(cuda, pts, nrm, images, disp, IDENTITY[None], focal), want, 'u = W - 1, w = 0, behind, NaN, inf, bad normals')
    for value in (0.0, -0.5, np.nan, np.inf, 0.5 * 1.06, 0.5 * 1.04):                 # one bad footprint pixel
        d = disp.copy()
        d[0, 21, 41] = value
        want = T.bake_points(pts, nrm, images, d, IDENTITY[None], focal)
        assert want[2][5] == (0 if value == 0.5 * 1.04 else -1)
        assert_bits(gpu_points(cuda, pts, nrm, images, d, IDENTITY[None], focal), want, f'disparity {value} at one footprint pixel')
    # a NaN and an infinite vertex in the atlas entry: their faces bake nothing, the others are untouched
    v, f, poses, sd, _, simg, _ = sphere_views()
    bad = v.copy()
    bad[f[40, 0]], bad[f[900, 1]] = (np.nan, 0, 0), (0, np.inf, 0)
    want = T.bake_atlas(bad, f, 3, simg, sd, poses, FOCAL)
    owner = T.owner_map(len(f), 3)[0]
    assert (want[2][(owner == 40) | (owner == 900)] == -1).all() and (want[2] >= 0).sum() > 1000
    assert_bits(gpu_atlas(cuda, bad, f, 3, simg, sd, poses), want, 'a NaN and an infinite vertex')
    for wrong in ([0, 1, len(v)], [0, -1, 2], [2 ** 31 - 1, 0, 1]):
        with pytest.raises(ValueError, match='face index'):
            gpu_atlas(cuda, v, np.concatenate([f, [wrong]]), 3, simg, sd, poses)
    with pytest.raises(ValueError, match='face index'):
        gpu_atlas(cuda, np.zeros((0, 3), np.float32), f[:4], 3, simg, sd, poses)


@pytest.mark.parametrize('h,w', [(1, 1), (1, 61), (37, 1), (9, 17)])
def test_smallest_images(h, w, cuda):
    """an image of one row or one column has 0 <= w <= 0 (0 <= u <= 0): only a point that projects exactly onto the row is inside,
    and none of these does; the textured resolve covers every shape."""
    one = np.asarray([TR.pixel_point(-50, -50, 2.0), TR.pixel_point(900, -40, 3.0), TR.pixel_point(-40, 700, 4.0)], np.float32)
    f = np.array([[0, 1, 2]], np.int32)
    disp, fmap, _ = N.rasterize(one, f, IDENTITY[None], h, w, FOCAL)
    images = np.random.RandomState(h + w).randint(0, 256, (1, h, w, 3)).astype(np.uint8)
    want = T.bake_atlas(one, f, 32, images, disp, IDENTITY[None], FOCAL, cull='none')
    assert (h > 1 and w > 1) or (want[2] == -1).all()
    assert_bits(gpu_atlas(cuda, one, f, 32, images, disp, IDENTITY[None], cull='none'), want, f'one triangle over an image of {h} x {w}')
    atlas = np.random.RandomState(h).randint(1, 256, T.atlas_uv(1, 32)[0]).astype(np.uint8)
    tex = T.texture_resolve(fmap, one, f, atlas, 32, IDENTITY[None], h, w, FOCAL)
    out = ops.mesh_texture_resolve(dev(fmap, cuda), dev(one, cuda), dev(f, cuda), dev(atlas, cuda), 32, dev(IDENTITY[None], cuda), FOCAL)
    assert np.array_equal(out.cpu().numpy(), tex) and (tex[fmap >= 0] > 0).all() and (fmap >= 0).sum() > 0


def test_texture_resolve_equals_the_restatement(cuda):
    v, f, poses, _, fmap, _, _ = sphere_views()
    for name, (vv, ff, pp, fm) in {'sphere': (v, f, poses, fmap), 'large and tiny': large_case()}.items():
        for n in (3, 8):
            shape = T.atlas_uv(len(ff), n)[0]
            atlas = np.random.RandomState(n).randint(0, 256, shape).astype(np.uint8)
            want = T.texture_resolve(fm, vv, ff, atlas, n, pp, H, W, FOCAL)
            args = (dev(fm, cuda), dev(vv, cuda), dev(ff, cuda), dev(atlas, cuda), n, dev(pp, cuda), FOCAL)
            got = ops.mesh_texture_resolve(*args)
            bad = int((got.cpu().numpy() != want).any(-1).sum())
            print(f'{name} at {n} texels: pixels that differ from the restatement: {bad} of {fm.size}; covered {int((fm >= 0).sum())}')
            assert got.dtype == torch.uint8 and got.shape == fm.shape + (3,) and bad == 0 and want[fm >= 0].any()
            assert (want[fm < 0] == 0).all() and torch.equal(got, ops.mesh_texture_resolve(*args))
    # a face map that names no face of the mesh gives 0
    wild = dev(np.full((1, H, W), len(f), np.int32), cuda)
    sevens = torch.full(T.atlas_uv(len(f), 8)[0], 7, device=cuda, dtype=torch.uint8)
    assert torch.all(ops.mesh_texture_resolve(wild, dev(v, cuda), dev(f, cuda), sevens, 8, dev(poses[:1], cuda), FOCAL) == 0)


def large_case():
    """the large-triangle case of tests/test_raster.py: vertices far outside the image, two poses."""
    v, f, col, _ = TR.large_and_tiny()
    poses = np.stack([IDENTITY, Wn.pose((0., 0., .02), (.05, -.03, .1))])
    fmap = TR.reference('large_and_tiny', v, f, poses, 'none', col)[1]
    return v, f, poses, fmap


def test_mesh_functions_equal_their_compositions(cuda, capsys):
    v, f, poses, disp, fmap, images, masks = sphere_views()
    hwf = (H, W, FOCAL)
    normals = R.vertex_normals(v, f).astype(np.float32)
    old = np.random.RandomState(4).randint(1, 256, v.shape).astype(np.uint8)
    m = mesh.Mesh(dev(v, cuda), dev(f, cuda), dev(normals, cuda), dev(old, cuda))
    two = poses[:2]
    # bake_texture: rasterise (cull off), bake
    tex = mesh.bake_texture(m, hwf, two, dev(images[:2], cuda), texels=4, masks=np.array(masks[:2]))
    want = T.bake_texture(v, f, 4, images[:2], two, H, W, FOCAL, masks=masks[:2])
    assert tex.texels == 4 and np.array_equal(tex.image.cpu().numpy(), want[0]) and np.array_equal(tex.seen.cpu().numpy(), want[1] > 0)
    assert np.array_equal(tex.uv, T.atlas_uv(len(f), 4)[1])
    owner = T.owner_map(len(f), 4)[0]
    unseen = int(((owner >= 0) & ~(want[1] > 0)).sum())
    assert f'{unseen} seen by no view' in capsys.readouterr().out and unseen > 0
    as_float = mesh.bake_texture(m, hwf, two, dev(images[:2], cuda).float() / 255.0, texels=4, masks=dev(masks[:2], cuda), verbose=False)
    assert torch.equal(as_float.image, tex.image)           # floats in 0..1 are the same bytes
    # the fill of unseen texels from the field: the head-on query of vertex_colors at the texel points
    asked = {}

    def query(pts, dirs, net):
        asked.setdefault('pts', []).append(pts[:, 0]), asked.setdefault('dirs', []).append(dirs)
        return torch.cat([2.0 * pts[:, 0], dirs[:, 2:3]], -1)[:, None]

    kw = {'network_fn': object(), 'network_fine': None, 'network_query_fn': query, 'use_viewdirs': True}
    filled = mesh.bake_texture(m, hwf, two, dev(images[:2], cuda), texels=4, masks=dev(masks[:2], cuda), render_kwargs=kw, chunk=5000, verbose=False)
    face, p, nrm, _ = T.atlas_points(v, f, 4)
    hole = (owner >= 0) & ~(want[1] > 0)
    got = filled.image.cpu().numpy()
    assert np.array_equal(got[~hole], want[0][~hole]) and torch.equal(filled.seen, tex.seen)
    expect = np.floor(255.0 / (1.0 + np.exp(-2.0 * p[hole])) + 0.5)
    assert np.abs(got[hole].astype(np.float64) - expect).max() <= 1          # fp32 points and sigmoid against fp64: one level
    ap, ad = torch.cat(asked['pts']).cpu().numpy(), torch.cat(asked['dirs']).cpu().numpy()
    unit = -nrm[hole] / np.linalg.norm(nrm[hole], axis=-1, keepdims=True)
    assert len(asked['pts']) == -(-int(hole.sum()) // 5000) and np.abs(ap - p[hole]).max() < 1e-6 and np.abs(ad - unit).max() < 1e-5
    # colors_from_views: baked at the vertices with the mesh's normals; unseen vertices keep their colour
    cm = mesh.colors_from_views(m, hwf, two, dev(images[:2], cuda))
    rgb, wsum, _ = T.bake_points(v, normals, images[:2], disp[:2], two, FOCAL)
    assert 0 < (wsum > 0).sum() < len(v)
    assert np.array_equal(cm.colors.cpu().numpy(), np.where((wsum > 0)[:, None], rgb, old)) and cm.verts is m.verts and cm.faces is m.faces
    bare = mesh.colors_from_views(mesh.Mesh(m.verts, m.faces, m.normals, None), hwf, two, dev(images[:2], cuda))
    assert np.array_equal(bare.colors.cpu().numpy(), np.where((wsum > 0)[:, None], rgb, 0))
    # render_textured: the rasteriser's maps and the textured resolve
    d3, f3, c3 = mesh.render_textured(m, tex, hwf, poses)
    w3 = T.render_textured(v, f, want[0], 4, poses, H, W, FOCAL)
    assert np.array_equal(d3.cpu().numpy().view(np.uint32), w3[0].view(np.uint32)) and np.array_equal(f3.cpu().numpy(), w3[1])
    assert np.array_equal(c3.cpu().numpy(), w3[2])
    back = mesh.render_textured(m, tex, hwf, poses, cull='back')
    assert np.array_equal(back[2].cpu().numpy(), T.render_textured(v, f, want[0], 4, poses, H, W, FOCAL, cull='back')[2])
    # mesh_image_metrics: coverage and PSNR from the restatement's render, SSIM = ops.ssim over the covered pixels
    region = masks[:2] | True
    region[0, :, :20] = False
    for texture, pred in ((tex, w3[2][:2]), (None, N.rasterize(v, f, two, H, W, FOCAL, colors=old)[2])):
        for reg in (None, region):
            rep = evaluate.mesh_image_metrics(m, texture, hwf, two, dev(images[:2], cuda), masks=None if reg is None else dev(reg, cuda))
            cov = (fmap[:2] >= 0) & (True if reg is None else reg)
            total = [H * W, H * W] if reg is None else [int(reg[k].sum()) for k in range(2)]
            assert rep['views'] == 2 and rep['per_view']['coverage'] == [int(cov[k].sum()) / total[k] for k in range(2)]
            x, y = pred.astype(np.float32) / np.float32(255), images[:2].astype(np.float32) / np.float32(255)
            for k in range(2):                              # fp32 means of about 1,400 squares: 1e-5 relative is generous
                mse = float(np.mean((x[k][cov[k]].astype(np.float64) - y[k][cov[k]]) ** 2))
                assert rep['per_view']['psnr'][k] == pytest.approx(-10.0 * math.log10(mse), rel=1e-5)
            # the images as the function scales them (a division by 255 on the device is not numpy's bit for bit)
            ssim = ops.ssim(dev(pred, cuda).float() / 255.0, dev(images[:2], cuda).float() / 255.0, mask=dev(cov, cuda)).cpu().tolist()
            assert rep['per_view']['ssim'] == ssim and rep['mean']['ssim'] == pytest.approx(np.mean(ssim))
    empty = evaluate.mesh_image_metrics(mesh.Mesh(m.verts, m.faces[:0], m.normals, m.colors), None, hwf, two, dev(images[:2], cuda))
    assert empty['per_view'] == {'coverage': [0.0, 0.0], 'psnr': [None, None], 'ssim': [None, None]}
    with pytest.raises(ValueError, match='images'):
        evaluate.mesh_image_metrics(m, tex, hwf, two, dev(images[:1], cuda))
    with pytest.raises(ValueError, match='texture'):
        evaluate.mesh_image_metrics(mesh.Mesh(m.verts, m.faces, m.normals, None), None, hwf, two, dev(images[:2], cuda))


def test_extract_mesh_tool_writes_a_textured_obj(cuda, tmp_path, capsys):
    """tools/extract_mesh.py --tsdf --fixture --texture on a field of two training iterations: OBJ + MTL + PNG of the mesh the tool
    reports, the atlas of its face count, from the field's renders and from the dataset's images."""
    import re
    from tools import extract_mesh as X
    for source in ('render', 'dataset'):
        out = str(tmp_path / f'{source}.obj')
        assert X.main(['--tsdf', '--fixture', '--iters', '2', '--view-step', '10', '--resolution', '24', '--out', out, '--texture', '4',
                       '--texture-from', source]) == 0
        text = capsys.readouterr().out
        m = re.search(r'tsdf zero level set: (\d+) vertices, (\d+) triangles', text)
        assert m and f'texture from 3 views' in text and 'seen by no view' in text
        nv, nf = int(m.group(1)), int(m.group(2))
        lines = open(out).read().splitlines()
        count = lambda key: sum(1 for line in lines if line.startswith(key + ' '))
        assert nf > 0 and (count('v'), count('vn'), count('vt'), count('f')) == (nv, nv, 3 * nf, nf)
        png = C.read_png(str(tmp_path / f'{source}.png'))
        assert png.shape == T.atlas_uv(nf, 4)[0] and png.any()
        assert f'map_Kd {source}.png' in open(str(tmp_path / f'{source}.mtl')).read()
    with pytest.raises(SystemExit):                        # a texture needs an OBJ to go with
        X.main(['--tsdf', '--fixture', '--out', str(tmp_path / 'x.ply'), '--texture', '4'])


def test_operand_checks(cuda):
    v, f, poses, disp, fmap, images, masks = sphere_views()
    tv, tf, tp, td, ti, tm = (dev(a, cuda) for a in (v, f, poses, disp, images, masks))
    tn = tv.clone()
    atlas = lambda a=tv, b=tf, n=3, i=ti, d=td, p=tp, focal=FOCAL, **kw: ops.mesh_bake_atlas(a, b, n, i, d, p, focal, **kw)
    points = lambda a=tv, b=tn, i=ti, d=td, p=tp, focal=FOCAL, **kw: ops.mesh_bake_points(a, b, i, d, p, focal, **kw)
    tfm = dev(fmap, cuda)
    ta = torch.zeros(T.atlas_uv(len(f), 3)[0], device=cuda, dtype=torch.uint8)
    resolve = lambda fm=tfm, a=tv, b=tf, t=ta, n=3, p=tp, focal=FOCAL, **kw: ops.mesh_texture_resolve(fm, a, b, t, n, p, focal, **kw)
    for call in (atlas, points):
        with pytest.raises(ValueError, match='no CPU path'):
            call(tv.cpu(), (tf if call is atlas else tn).cpu())
        for name, bad in (('i', ti.cpu()), ('d', td.cpu()), ('p', tp.cpu())):
            with pytest.raises(ValueError, match='no CPU path'):
                call(**{name: bad})
        with pytest.raises(ValueError, match='no CPU path'):
            call(masks=tm.cpu())
        with pytest.raises(ValueError, match='must be torch.float32'):
            call(tv.double())
        with pytest.raises(ValueError, match='must be torch.float32'):
            call(d=td.double())
        with pytest.raises(ValueError, match='must be torch.float32'):
            call(p=tp.double())
        with pytest.raises(ValueError, match='torch.uint8'):
            call(i=ti.float())
        with pytest.raises(ValueError, match='must be torch.bool'):
            call(masks=tm.to(torch.uint8))
        with pytest.raises(ValueError, match=r'\[N, 3, 4\]'):
            call(p=tp[:, :, :3].contiguous())
        with pytest.raises(ValueError, match='one V, H, W'):
            call(i=ti[:2].contiguous())
        with pytest.raises(ValueError, match='one V, H, W'):
            call(d=td[:, :-1].contiguous())
        with pytest.raises(ValueError, match='one V, H, W'):
            call(masks=tm[:, :, :-1].contiguous())
        with pytest.raises(ValueError, match='one V, H, W'):
            call(p=tp[:2].contiguous())
        with pytest.raises(ValueError, match='contiguous'):
            call(d=td.transpose(1, 2).contiguous().transpose(1, 2))
        with pytest.raises(ValueError, match='tensor on the GPU'):
            call(v)
        for bad in (0.0, -1.0, float('nan'), float('inf')):
            with pytest.raises(ValueError, match='finite and > 0'):
                call(focal=bad)
            with pytest.raises(ValueError, match='finite and > 0'):
                call(near=bad)
        for bad in (-1e-3, float('nan'), float('inf')):
            with pytest.raises(ValueError, match='tol'):
                call(tol=bad)
        with pytest.raises(ValueError, match='cull'):
            call(cull='front')
        with pytest.raises(ValueError, match='mode'):
            call(mode='mean')
    with pytest.raises(ValueError, match='must be torch.int32'):
        atlas(b=tf.long())
    with pytest.raises(ValueError, match=r'\[F, 3\]'):
        atlas(b=tf[:, :2].contiguous())
    for bad in (0, 33, 2.5):
        with pytest.raises(ValueError, match='texels'):
            atlas(n=bad)
    with pytest.raises(ValueError, match='order'):
        atlas(order='column')
    with pytest.raises(ValueError, match='one shape'):
        points(b=tn[:5].contiguous())
    with pytest.raises(ValueError, match=r'\[N, 3\]'):
        points(tv.reshape(-1), tn.reshape(-1))
    with pytest.raises(ValueError, match='no CPU path'):
        resolve(tfm.cpu())
    with pytest.raises(ValueError, match='no CPU path'):
        resolve(t=ta.cpu())
    with pytest.raises(ValueError, match='must be torch.int32'):
        resolve(tfm.long())
    with pytest.raises(ValueError, match='atlas'):
        resolve(t=ta[:-1].contiguous())
    with pytest.raises(ValueError, match='atlas'):
        resolve(t=ta.float())
    with pytest.raises(ValueError, match='atlas'):
        resolve(n=4)
    with pytest.raises(ValueError, match='one V'):
        resolve(p=tp[:2].contiguous())
    with pytest.raises(ValueError, match='texels'):
        resolve(n=0)
    with pytest.raises(ValueError, match='finite and > 0'):
        resolve(focal=0.0)
    with pytest.raises(ValueError, match='a side over'):
        ops.texture_layout(2 * 2341 ** 2 + 1, 4)


def test_abi_refuses_before_any_device_call(cuda):
    lib = _lib.load()
    buf = torch.zeros(4096, device=cuda, dtype=torch.int32)
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(buf.data_ptr())
    st = _lib.stream()
    big, nan, inf = 2 ** 31, float('nan'), float('inf')
    view_changes = lambda k: [(k, null), (k + 1, null), (k + 3, null), (k + 4, -1), (k + 4, big), (k + 5, 0), (k + 5, 16385), (k + 6, 0),
                              (k + 6, 16385), (k + 7, 0.0), (k + 7, -1.0), (k + 7, nan), (k + 7, inf), (k + 8, 0.0), (k + 8, nan),
                              (k + 8, inf), (k + 9, -1e-3), (k + 9, nan), (k + 9, inf), (k + 10, 2), (k + 10, -1), (k + 11, 2), (k + 11, -1)]
    # (points, normals, N, images, disp, masks, poses, V, H, W, focal, near, tol, cull, mode, rgb, wsum, best)
    good = [one, one, 8, one, one, null, one, 1, 4, 4, 1.0, 1e-3, 0.05, 1, 0, one, one, one]
    for k, value in [(0, null), (1, null), (2, -1), (15, null), (16, null), (17, null)] + view_changes(3):
        args = list(good)
        args[k] = value
        assert lib.mvip_texture_bake_points(*args, st) == -1, (k, value)
    # (verts, faces, Nv, F, texels, order, images, disp, masks, poses, V, H, W, focal, near, tol, cull, mode, rgb, wsum, best, flag)
    good = [one, one, 3, 1, 4, 0, one, one, null, one, 1, 4, 4, 1.0, 1e-3, 0.05, 1, 0, one, one, one, one]
    changes = [(0, null), (1, null), (2, -1), (2, big), (3, -1), (3, big // 3 + 1), (4, 0), (4, 33), (4, -1), (5, 2), (5, -1), (18, null),
               (19, null), (20, null), (21, null), (3, 2 * 2341 ** 2 + 1)] + view_changes(6)
    for k, value in changes:
        args = list(good)
        args[k] = value
        assert lib.mvip_texture_bake_atlas(*args, st) == -1, (k, value)
    # (face, verts, faces, Nv, F, atlas, texels, poses, V, H, W, focal, near, rgb)
    good = [one, one, one, 3, 1, one, 4, one, 1, 4, 4, 1.0, 1e-3, one]
    changes = [(0, null), (1, null), (2, null), (5, null), (7, null), (13, null), (3, -1), (3, big), (4, -1), (4, big // 3 + 1), (6, 0), (6, 33),
               (8, -1), (8, big), (9, 0), (9, 16385), (10, 0), (10, 16385), (11, 0.0), (11, nan), (11, inf), (12, 0.0), (12, nan), (12, inf),
               (4, 2 * 2341 ** 2 + 1)]
    for k, value in changes:
        args = list(good)
        args[k] = value
        assert lib.mvip_texture_resolve(*args, st) == -1, (k, value)
    torch.cuda.synchronize()
    assert int(buf.abs().sum()) == 0                        # nothing was written
