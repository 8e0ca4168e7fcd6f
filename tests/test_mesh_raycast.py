"""Mesh ray casting on the GPU (csrc/mesh_raycast.hip) against its brute-force restatement tests/mesh_raycast_numpy.py: first
hits on the face grid (face, t and bary BIT-EQUAL on every grid: the result must not depend on the grid), occlusion, skip, face
openness, mesh.cast_rays / cast_views / drop_interior, the argument checks of ops."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_raycast_numpy as C                           # noqa: E402

from mvip_nerf_amd import mesh, ops                      # noqa: E402

pytestmark = pytest.mark.gpu

F32, F64, I32 = np.float32, np.float64, np.int32
_cache = {}


def once(key, make):
    """a mesh, a ray set or a brute-force answer, made once and left unchanged"""
    if key not in _cache:
        out = make()
        for a in out:
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _cache[key] = out
    return _cache[key]


def dev(cuda, *arrays):
    return [torch.from_numpy(np.array(a)).to(cuda) for a in arrays]                        # (a writable copy)


def sphere_rays():
    """about 3 k rays for the 1,280-face icosphere: from inside, from outside, missing the box entirely, from 10^4 box diagonals
    away, through vertices, some with tmin / tmax cuts, invalid ones of every kind interleaved; N is no multiple of 64"""
    v, _ = C.icosphere(3)
    rng = np.random.default_rng(1)

    def unit(n):
        x = rng.standard_normal((n, 3))
        return x / np.linalg.norm(x, axis=1, keepdims=True)
    diag = float(np.linalg.norm(v.max(0) - v.min(0)))
    oi, di = rng.uniform(-0.5, 0.5, (700, 3)), unit(700)
    oo = 3 * unit(900)
    do = -oo + 0.8 * rng.standard_normal((900, 3))
    om = 3 * unit(300)
    dm = np.cross(om, unit(300))                                                          # tangential: these miss the box
    far = 1e4 * diag * unit(500)
    df = (rng.uniform(-0.8, 0.8, (500, 3)) - far) / 1e4                                    # aimed at points of the box
    ov = np.tile(np.asarray([[0.3, -0.2, 0.1]]), (600, 1))
    dv = v[rng.choice(len(v), 600)] - ov                                                  # exactly through vertices
    o, d = np.concatenate([oi, oo, om, far, ov]).astype(F32), np.concatenate([di, do, dm, df, dv]).astype(F32)
    tmin, tmax = np.zeros(len(o), F32), np.full(len(o), np.inf, F32)
    tmax[::7], tmin[::11] = 2.5, 0.7
    for j, i in enumerate(range(5, len(o), 97)):
        k = j % 6
        if k == 0:
            o[i, 0] = np.nan
        elif k == 1:
            d[i] = 0
        elif k == 2:
            d[i, 1] = np.inf
        elif k == 3:
            tmin[i] = -np.inf
        elif k == 4:
            tmax[i] = np.nan
        else:
            tmin[i], tmax[i] = 2, 1
    assert len(o) == 3000 and len(o) % 64 != 0
    return o, d, tmin, tmax


def degenerate_mesh():
    """the icosphere plus: one triangle spanning the whole box, a face entered twice more, faces that repeat a vertex, a point
    face, an unreferenced vertex"""
    v, f = C.icosphere(3)
    V = len(v)
    ev = np.asarray([[-1, -1, -1], [1, 1, -1], [0, 0, 1], [0.3, 0.3, 0.3]], F32)
    ef = np.asarray([[V, V + 1, V + 2], f[7], f[7], [f[9, 0], f[9, 1], f[9, 0]], [f[11, 2]] * 3, [V, V, V + 1]], I32)
    return np.concatenate([v, ev]), np.concatenate([f[:40], ef, f[40:]]).astype(I32)


def same(got, ref, what=''):
    face, t = got[0].cpu().numpy(), got[1].cpu().numpy()
    assert face.dtype == I32 and t.dtype == F32
    np.testing.assert_array_equal(face, ref[0], err_msg=what + ' face')
    np.testing.assert_array_equal(t, ref[1], err_msg=what + ' t')                            # NaN == NaN, inf == inf here
    if len(got) > 2 and got[2] is not None and got[2].dtype == torch.float32:
        np.testing.assert_array_equal(got[2].cpu().numpy(), ref[2], err_msg=what + ' bary')


def check_case(cuda, vn, fn, rays, ref, grids, what):
    v, f, o, d, tmin, tmax = dev(cuda, vn, fn, *rays)
    hit = ref[0] >= 0
    tests = {}
    for cells in grids:
        grid = ops.mesh_face_grid(v, f, cells=cells)
        got = ops.mesh_cast_rays(o, d, v, f, tmin=tmin, tmax=tmax, grid=grid, return_bary=True, return_stats=True)
        same(got, ref, f'{what} cells={cells}')
        n_tests, slots, n_cells = (int(x) for x in got[3].cpu())
        assert 0 < n_tests <= slots <= 64 * n_tests and n_cells > 0
        tests[cells] = n_tests
        occ = ops.mesh_occluded(o, d, v, f, tmin=tmin, tmax=tmax, grid=grid)
        assert occ.dtype == torch.bool
        np.testing.assert_array_equal(occ.cpu().numpy(), hit, err_msg=f'{what} cells={cells} occluded')
    same(ops.mesh_cast_rays(o, d, v, f, tmin=tmin, tmax=tmax), ref, what + ' grid built inside')
    return tests


def test_lattice_aligned_mesh_on_six_grids(cuda):
    vn, fn = once('lattice', C.lattice_mesh)
    rays = once('lattice rays', C.lattice_rays)
    ref = once('lattice ref', lambda: C.cast_rays(*rays, vn, fn))
    assert 300 < (ref[0] >= 0).sum() < 1000
    tests = check_case(cuda, vn, fn, rays, ref, (1, (4, 4, 2), (8, 8, 4), (3, 5, 7), 16, None), 'lattice')
    print('ray-face tests per ray:', {k: round(t / len(rays[0]), 2) for k, t in tests.items()})
    assert tests[16] < tests[(4, 4, 2)] < tests[1] <= len(rays[0]) * len(fn)


def test_icosphere_inside_outside_missing_far_and_invalid_rays(cuda):
    vn, fn = once('sphere', lambda: C.icosphere(3))
    rays = once('sphere rays', sphere_rays)
    ref = once('sphere ref', lambda: C.cast_rays(*rays, vn, fn))
    face, t = ref[0], ref[1]
    invalid = ~C.valid_rays(*rays)
    assert invalid.sum() >= 30 and np.all(face[invalid] == -1) and np.all(np.isnan(t[invalid]))
    assert np.all(face[1600:1900][~invalid[1600:1900]] == -1)                              # the tangential ones
    assert (face[1900:2400] >= 0).sum() > 300                                               # the far ones
    assert np.all(np.isinf(t[(face < 0) & ~invalid]))
    tests = check_case(cuda, vn, fn, rays, ref, (None, 1, 5, (16, 3, 7)), 'icosphere')
    print('ray-face tests per ray:', {k: round(t / 3000, 2) for k, t in tests.items()}, 'faces', len(fn))
    assert tests[None] < tests[5] < tests[1]


def test_degenerate_and_duplicate_faces(cuda):
    vn, fn = once('degenerate', degenerate_mesh)
    rays = once('sphere rays', sphere_rays)
    ref = once('degenerate ref', lambda: C.cast_rays(*rays, vn, fn))
    assert 40 in ref[0] and 7 in ref[0]                                                    # the spanning face and the repeated face are hit,
    assert not np.isin(ref[0], [41, 42, 43, 44, 45]).any()                                # its later copies and the degenerate ones never
    check_case(cuda, vn, fn, rays, ref, (None, 3), 'degenerate')


def test_skip_removes_exactly_the_skipped_face(cuda):
    vn, fn = once('sphere', lambda: C.icosphere(3))
    rays = once('sphere rays', sphere_rays)
    first = once('sphere ref', lambda: C.cast_rays(*rays, vn, fn))
    skip = first[0].copy()
    skip[::5] = 3                                                                           # some other face, mostly not on the ray
    ref = once('sphere skip ref', lambda: C.cast_rays(*rays, vn, fn, skip=skip))
    changed = ref[0] != first[0]
    assert changed.sum() > 1000 and np.all(first[0][changed] == skip[changed])              # only rays whose own hit was skipped
    assert np.all((ref[0] != skip) | (ref[0] < 0))
    v, f, o, d, tmin, tmax, sk = dev(cuda, vn, fn, *rays, skip)
    same(ops.mesh_cast_rays(o, d, v, f, tmin=tmin, tmax=tmax, skip=sk, return_bary=True), ref, 'skip')
    occ = ops.mesh_occluded(o, d, v, f, tmin=tmin, tmax=tmax, skip=sk)
    np.testing.assert_array_equal(occ.cpu().numpy(), ref[0] >= 0)
    none = torch.full_like(sk, -1)
    same(ops.mesh_cast_rays(o, d, v, f, tmin=tmin, tmax=tmax, skip=none), first, 'skip -1')


def test_scalar_limits_and_ray_arrays_of_length_zero_one_and_1025(cuda):
    vn, fn = once('sphere', lambda: C.icosphere(3))
    o_, d_, _, _ = once('sphere rays', sphere_rays)
    ref = once('sphere scalar ref', lambda: C.cast_rays(o_[:1025], d_[:1025], 0.25, 3.5, vn, fn))
    v, f, o, d = dev(cuda, vn, fn, o_[:1025], d_[:1025])
    grid = ops.mesh_face_grid(v, f)
    same(ops.mesh_cast_rays(o, d, v, f, tmin=0.25, tmax=3.5, grid=grid, return_bary=True), ref)
    same(ops.mesh_cast_rays(o[:1].contiguous(), d[:1].contiguous(), v, f, tmin=0.25, tmax=3.5, grid=grid), tuple(r[:1] for r in ref))
    empty = ops.mesh_cast_rays(o[:0].contiguous(), d[:0].contiguous(), v, f, grid=grid, return_bary=True)
    assert [tuple(t.shape) for t in empty] == [(0,), (0,), (0, 2)]
    assert tuple(ops.mesh_occluded(o[:0].contiguous(), d[:0].contiguous(), v, f).shape) == (0,)


def test_openness_of_nested_spheres_and_drop_interior(cuda):
    vn, fn, n_outer = once('nested', lambda: C.nested_spheres(2))
    dirs = C.fibonacci_directions(16)
    ref = once('nested ref', lambda: C.face_openness(vn, fn, dirs))
    v, f, dd = dev(cuda, vn, fn, dirs)
    got = ops.mesh_face_openness(v, f, dd, return_stats=True)
    for g, r, name in zip(got, ref, ('front_open', 'front_total', 'back_open', 'back_total')):
        assert g.dtype == torch.int32
        np.testing.assert_array_equal(g.cpu().numpy(), r, err_msg=name)
    n_tests, slots, n_cells = (int(x) for x in got[4].cpu())
    assert 0 < n_tests <= slots <= 64 * n_tests and n_cells > 0
    fo, ft, bo, bt = (g.cpu().numpy() for g in got[:4])
    assert np.array_equal(fo[:n_outer], ft[:n_outer]) and not bo[:n_outer].any() and not fo[n_outer:].any() and not bo[n_outer:].any()
    near = once('nested near ref', lambda: C.face_openness(vn, fn, dirs, max_dist=0.3))
    for g, r in zip(ops.mesh_face_openness(v, f, dd, max_dist=0.3, grid=ops.mesh_face_grid(v, f, cells=4)), near):
        np.testing.assert_array_equal(g.cpu().numpy(), r)
    m = mesh.Mesh(v, f, None, None)
    for g, r in zip(mesh.face_openness(m, 16), ref):                                        # the Python layer's own Fibonacci set
        np.testing.assert_array_equal(g.cpu().numpy(), r)
    for two_sided in (True, False):
        kept = mesh.drop_interior(m, directions=16, two_sided=two_sided)
        np.testing.assert_array_equal(kept.faces.cpu().numpy(), fn[:n_outer])               # exactly the outer sphere, in order
        np.testing.assert_array_equal(kept.verts.cpu().numpy(), vn[:len(vn) // 2])
    # an open sheet seen from behind: two_sided keeps it, front-only keeps what faces outwards
    flipped = mesh.Mesh(v, f[:, [0, 2, 1]].contiguous(), None, None)
    assert mesh.drop_interior(flipped, 16, two_sided=True).faces.shape[0] == n_outer
    assert mesh.drop_interior(flipped, 16, two_sided=False).faces.shape[0] == 0
    e = torch.empty((0, 3), device=cuda, dtype=torch.int32)
    assert [tuple(t.shape) for t in ops.mesh_face_openness(v, e, dd)] == [(0,)] * 4


H, W, FOCAL = 12, 16, 14.0
IDENTITY = np.asarray([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]], F32)


def test_cast_rays_on_get_rays_rows_gives_the_planar_disparity(cuda):
    """a camera at the origin looking down -z at the plane z = -2 (and a second one, turned and moved): the ray parameter of
    get_rays rows is the planar depth, so the disparity is fp32(1 / t) with t the restatement's"""
    vn = np.asarray([[-9, -9, -2], [9, -9, -2], [9, 9, -2], [-9, 9, -2]], F32)
    fn = np.asarray([[0, 1, 2], [0, 2, 3]], I32)
    v, f = dev(cuda, vn, fn)
    m = mesh.Mesh(v, f, None, None)
    c, s = np.cos(0.3), np.sin(0.3)
    turned = np.asarray([[c, 0, s, 0.2], [0, 1, 0, -0.1], [-s, 0, c, 0.4]], F32)
    for pose, cols in ((IDENTITY, 11), (turned, 8)):
        ro, rd = ops.get_rays(H, W, FOCAL, torch.from_numpy(pose).to(cuda))
        rows = ops.ray_rows(ro, rd, 0.5, 6.0, viewdirs_src=rd)
        rows = rows[:, :cols].contiguous()
        face, depth, disp = mesh.cast_rays(m, rows)
        rn = rows.cpu().numpy()
        ref = C.cast_rays(rn[:, 0:3], rn[:, 3:6], rn[:, 6], rn[:, 7], vn, fn)
        same((face, depth), ref)
        assert np.all(ref[0] >= 0)
        want = (1.0 / ref[1].astype(F64)).astype(F32)
        np.testing.assert_array_equal(disp.cpu().numpy(), want)
        if pose is IDENTITY:
            assert np.all(ref[1] == 2.0) and np.all(want == 0.5)
        else:                                                                               # the planar depth along the camera's axis
            p = rn[:, 0:3].astype(F64) + ref[3][:, None] * rn[:, 3:6].astype(F64)
            z_cam = -(p - pose[:, 3].astype(F64)) @ pose[:, 2].astype(F64)
            np.testing.assert_allclose(ref[1], z_cam, rtol=1e-6)
    rows[:, 7] = 1.0                                                                        # far in front of the plane: nothing
    face, depth, disp = mesh.cast_rays(m, rows)
    assert bool((face == -1).all()) and bool(torch.isinf(depth).all()) and bool((disp == 0).all())
    with pytest.raises(ValueError, match='rows'):
        mesh.cast_rays(m, rows[:, :7].contiguous())


def test_cast_views_sees_a_quad_that_crosses_the_near_plane(cuda):
    """a floor quad from behind the camera to z = -6: the rasteriser drops it whole (a vertex nearer than `near`), the ray cast
    sees it beyond the near plane, with the interpolated colours"""
    vn = np.asarray([[-4, -0.5, 1], [4, -0.5, 1], [4, -0.5, -6], [-4, -0.5, -6]], F32)
    fn = np.asarray([[0, 1, 2], [0, 2, 3]], I32)
    cn = np.asarray([[200, 0, 0], [200, 0, 0], [0, 100, 50], [0, 100, 50]], np.uint8)
    v, f, c = dev(cuda, vn, fn, cn)
    m = mesh.Mesh(v, f, None, c)
    poses = torch.from_numpy(IDENTITY[None]).to(cuda)
    near, far = 0.25, 10.0
    _, rface, _ = mesh.render_views(m, (H, W, FOCAL), poses, near=near)
    assert bool((rface == -1).all())
    disp, face, rgb = mesh.cast_views(m, (H, W, FOCAL), poses, near, far)
    assert disp.shape == (1, H, W) and face.shape == (1, H, W) and rgb.shape == (1, H, W, 3) and rgb.dtype == torch.uint8
    ro, rd = ops.get_rays(H, W, FOCAL, poses[0])
    on, dn = ro.reshape(-1, 3).cpu().numpy(), rd.reshape(-1, 3).cpu().numpy()
    ref = C.cast_rays(on, dn, near, far, vn, fn)
    np.testing.assert_array_equal(face.reshape(-1).cpu().numpy(), ref[0])
    hit = ref[0] >= 0
    want = np.where(hit, (1.0 / ref[1].astype(F64)).astype(F32), F32(0))
    np.testing.assert_array_equal(disp.reshape(-1).cpu().numpy(), want)
    rows_hit = hit.reshape(H, W).any(1)
    assert not rows_hit[:H // 2 + 1].any() and rows_hit[H // 2 + 2:].all()                    # the floor: below the horizon only
    depth = ref[1][hit]
    assert depth.min() >= near and depth.max() <= 6.0
    # colours: linear in the world z of the hit
    z = (on + np.where(hit, ref[3], 0.0)[:, None] * dn)[:, 2]
    w_far = np.clip((1.0 - z) / 7.0, 0, 1)
    want_rgb = np.stack([200 * (1 - w_far), 100 * w_far, 50 * w_far], 1)
    got_rgb = rgb.reshape(-1, 3).cpu().numpy().astype(F64)
    assert np.abs(got_rgb[hit] - want_rgb[hit]).max() <= 0.5 + 1e-3 and not got_rgb[~hit].any()
    assert mesh.cast_views(m, (H, W, FOCAL), poses, near, far, colors=False)[2] is None


def test_ops_reject_bad_arguments(cuda):
    vn, fn = once('sphere', lambda: C.icosphere(3))
    v, f = dev(cuda, vn, fn)
    o = torch.zeros((10, 3), device=cuda)
    d = torch.ones((10, 3), device=cuda)
    grid = ops.mesh_face_grid(v, f)
    lim = torch.ones(10, device=cuda)
    for bad in (dict(origins=o.double()), dict(origins=o.cpu()), dict(origins=o[:, :2].contiguous()), dict(origins=o.t()[:, :3]),
                dict(origins=vn[:10]), dict(dirs=d[:9].contiguous()), dict(dirs=d.half()), dict(verts=v.cpu()), dict(faces=f.long()),
                dict(faces=f[:0].contiguous()), dict(tmin=lim[:9].contiguous()), dict(tmax=lim.double()), dict(tmin='0'),
                dict(tmax=float('nan')), dict(skip=lim), dict(skip=torch.zeros(9, device=cuda, dtype=torch.int32)), dict(grid='grid'),
                dict(grid=ops.mesh_face_grid(v.clone(), f))):
        args = dict(origins=o, dirs=d, verts=v, faces=f)
        args.update(bad)
        with pytest.raises(ValueError):
            ops.mesh_cast_rays(**args)
        with pytest.raises(ValueError):
            ops.mesh_occluded(**args)
    ops.mesh_cast_rays(o, d, v, f, tmin=lim, tmax=2.0, grid=grid)
    dirs = torch.from_numpy(C.fibonacci_directions(8)).to(cuda)
    nan_dir = dirs.clone()
    nan_dir[3, 1] = float('nan')
    for bad in (dict(directions=dirs.cpu()), dict(directions=dirs[:, :2].contiguous()), dict(directions=nan_dir),
                dict(directions=torch.ones((256, 3), device=cuda)), dict(max_dist=-1.0), dict(max_dist=float('nan')),
                dict(grid=ops.mesh_face_grid(v.clone(), f)), dict(faces=f.long())):
        args = dict(verts=v, faces=f, directions=dirs)
        args.update(bad)
        with pytest.raises(ValueError):
            ops.mesh_face_openness(**args)
    f_bad = f.clone()
    f_bad[5, 1] = len(vn)
    with pytest.raises(ValueError, match='outside'):
        ops.mesh_cast_rays(o, d, v, f_bad)
    with pytest.raises(ValueError, match='keep|directions|count'):
        mesh.face_openness(mesh.Mesh(v, f, None, None), 300)


def test_extract_mesh_tool_drops_interior_faces(cuda, tmp_path, capsys):
    """tools/extract_mesh.py --drop-interior K on a tiny synthetic model (seeded weights, 24^3 lattice): the file is, byte for
    byte, what extract_mesh + drop_interior + save_ply write, and the counts are printed."""
    from oracle.weights import seeded_state_dict
    from tools import extract_mesh as T
    ckpt = str(tmp_path / 'tiny.tar')
    torch.save({'global_step': 0,
                'network_fn_state_dict': {k: torch.from_numpy(w) for k, w in seeded_state_dict(2).items()},
                'network_fine_state_dict': {k: torch.from_numpy(w) for k, w in seeded_state_dict(1).items()}}, ckpt)
    kw, _ = T.load_model(ckpt, 'mlp', cuda)
    lo, hi, res = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0), 24
    thr = float(mesh.density_grid(kw, lo, hi, res).median())
    tool, direct = str(tmp_path / 'tool.ply'), str(tmp_path / 'direct.ply')
    assert T.main([ckpt, '--resolution', str(res), '--threshold', repr(thr), '--out', tool, '--drop-interior', '16']) == 0
    m = mesh.extract_mesh(kw, lo, hi, resolution=res, threshold=thr)
    kept = mesh.drop_interior(m, directions=16)
    mesh.save_ply(direct, kept)
    assert open(tool, 'rb').read() == open(direct, 'rb').read()
    assert 0 < kept.faces.shape[0] <= m.faces.shape[0]
    line = [ln for ln in capsys.readouterr().out.split('\n') if ln.startswith('open in at least one of 16 directions: ')]
    assert len(line) == 1 and f'{m.faces.shape[0]} triangles' in line[0] and f'-> {kept.faces.shape[0]} triangles' in line[0]
    with pytest.raises(SystemExit):
        T.main([ckpt, '--out', tool, '--drop-interior', '256'])
