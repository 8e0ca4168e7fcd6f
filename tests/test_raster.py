"""The mesh rasteriser on the GPU (csrc/raster.hip, ops.mesh_rasterize) against its restatement tests/raster_numpy.py: the bits of
disp, face and rgb must be EQUAL EVERYWHERE -- the definition is fp64 and integers, there is no tolerance and nothing is excluded
-- and a repetition must be bit-equal.  Then mesh.render_views / visible_faces / keep_faces, evaluate.mesh_depth_metrics, the
argument checks of ops and of the C ABI."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mc_numpy as M                                     # noqa: E402
import mesh_ops_numpy as R                               # noqa: E402
import raster_numpy as N                                 # noqa: E402
import warp_numpy as Wn                                  # noqa: E402
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench                                             # noqa: E402
from mvip_nerf_amd import _lib, evaluate, mesh, ops, run  # noqa: E402

pytestmark = pytest.mark.gpu

H, W, FOCAL = 48, 64, 60.0
SPHERE_POSES = (((0., 0., 0.), (0., 0., 3.)), ((.1, .5, .05), (1.6, -.3, 2.6)), ((0., 0., 0.), (0., 0., .3)))
IDENTITY = Wn.pose()
_cache = {}


def sphere():
    if 'sphere' not in _cache:
        v, f, _ = M.marching_cubes(R.lattice(24, R.sphere_field()), 1.0, R.LO, R.HI)
        col = np.random.RandomState(11).randint(0, 256, v.shape).astype(np.uint8)
        for a in (v, f, col):
            a.setflags(write=False)
        _cache['sphere'] = (v, f.astype(np.int32), col)
    return _cache['sphere']


def sphere_poses():
    return np.stack([Wn.pose(a, o) for a, o in SPHERE_POSES])


def reference(name, verts, faces, poses, cull, colors, h=H, w=W):
    """the restatement's maps of a named case, computed once."""
    key = (name, cull, colors is not None)
    if key not in _cache:
        out = N.rasterize(verts, faces, poses, h, w, FOCAL, cull=cull, colors=colors)
        for a in out:
            if a is not None:
                a.setflags(write=False)
        _cache[key] = out
    return _cache[key]


def dev(a, cuda):
    return torch.from_numpy(np.array(a, order='C')).to(cuda)         # a copy: the cached arrays are read-only


def gpu(cuda, verts, faces, poses, cull='none', colors=None, h=H, w=W, **kw):
    out = ops.mesh_rasterize(dev(np.asarray(verts, np.float32), cuda), dev(np.asarray(faces, np.int32).reshape(-1, 3), cuda),
                             dev(np.asarray(poses, np.float32).reshape(-1, 3, 4), cuda), h, w, FOCAL, cull=cull,
                             colors=None if colors is None else dev(colors, cuda), **kw)
    disp, face, rgb = out[:3]
    V = np.asarray(poses).reshape(-1, 3, 4).shape[0]
    assert disp.dtype == torch.float32 and face.dtype == torch.int32 and disp.shape == face.shape == (V, h, w)
    assert (rgb is None) == (colors is None) and (rgb is None or (rgb.dtype == torch.uint8 and rgb.shape == (V, h, w, 3)))
    return out


def assert_equal_everywhere(got, want, what):
    disp, face, rgb = got[:3]
    d, f = disp.cpu().numpy(), face.cpu().numpy()
    nd, nf = int((d.view(np.uint32) != want[0].view(np.uint32)).sum()), int((f != want[1]).sum())
    nc = 0 if want[2] is None else int((rgb.cpu().numpy() != want[2]).any(-1).sum())
    print(f'{what}: pixels that differ from the restatement: disp {nd}, face {nf}, rgb {nc} of {d.size}; covered {int((want[1] >= 0).sum())}')
    assert nd == 0 and nf == 0 and nc == 0


@pytest.mark.parametrize('cull', N.CULLS)
@pytest.mark.parametrize('coloured', [False, True])
def test_sphere_views_equal_the_restatement(cull, coloured, cuda):
    v, f, col = sphere()
    assert len(f) > 1024 and len(f) % 256 != 0              # past one workgroup and no multiple of it
    col = col if coloured else None
    want = reference('sphere', v, f, sphere_poses(), cull, col)
    assert [int((want[1][i] >= 0).sum()) for i in range(3)] == ([481, 450, 3072] if cull == 'none' else [481, 450, 0])
    got = gpu(cuda, v, f, sphere_poses(), cull, col)
    assert_equal_everywhere(got, want, f'sphere, 3 views, cull {cull}, colours {coloured}')
    again = gpu(cuda, v, f, sphere_poses(), cull, col)
    for a, b in zip(got, again):
        assert a is None or torch.equal(a.view(torch.uint8), b.view(torch.uint8))


def pixel_point(u, w, z):
    """the world point that the identity camera sees at pixel (u, w) and planar depth z."""
    return [(u - W / 2) * z / FOCAL, -(w - H / 2) * z / FOCAL, -z]


def large_and_tiny():
    """four triangles that each cover more than half of the image, with vertices outside it (one 1,500 pixels away), mixed with
    200 tiny ones so that both paths of the fragment kernel run in the same waves."""
    big = [[(-10, -10, 3.0), (1500, -5, 4.0), (-8, 90, 5.0)], [(70, -20, 2.5), (70, 60, 6.0), (-40, 20, 3.5)],
           [(-20, -5, 5.5), (90, 20, 2.2), (-20, 60, 4.5)], [(-6, -6, 4.2), (80, -6, 3.1), (30, 200, 2.9)]]
    rs = np.random.RandomState(21)
    verts, faces = [], []
    slots = {10, 70, 130, 190}
    for n in range(204):
        if n in slots:
            tri = big[len([s for s in slots if s < n])]
        else:
            cx, cy, z = rs.uniform(-2, W + 2), rs.uniform(-2, H + 2), rs.uniform(2.0, 6.0)
            tri = [(cx + dx, cy + dy, z + dz) for dx, dy, dz in rs.uniform(-1.6, 1.6, (3, 3)) * [1, 1, .1]]
        faces.append([len(verts), len(verts) + 1, len(verts) + 2])
        verts += [pixel_point(*p) for p in tri]
    col = rs.randint(0, 256, (len(verts), 3)).astype(np.uint8)
    return np.asarray(verts, np.float32), np.asarray(faces, np.int32), col, sorted(slots)


def test_wave_cooperative_path_mixed_with_tiny_faces(cuda):
    v, f, col, slots = large_and_tiny()
    poses = np.stack([IDENTITY, Wn.pose((0., 0., .02), (.05, -.03, .1))])
    for s in slots:                                        # each large face alone covers more than half of the image
        alone = N.rasterize_view(v, f[s:s + 1], IDENTITY, H, W, FOCAL)
        assert (alone['face'] >= 0).sum() > H * W // 2
    X = N.project(v, IDENTITY, H, W, FOCAL, 1e-3)[0]
    assert X.max() > 1000 * 256
    for cull in N.CULLS:
        want = reference('large_and_tiny', v, f, poses, cull, col)
        winners = set(np.unique(want[1][want[1] >= 0]))
        assert cull == 'back' or (winners & set(slots) and winners - set(slots))    # both kinds win pixels
        got = gpu(cuda, v, f, poses, cull, col)
        assert_equal_everywhere(got, want, f'4 large + 200 tiny faces, cull {cull}')
    # a single triangle over the whole image of the largest tile-unfriendly shape: one row, one column
    one = np.asarray([pixel_point(-50, -50, 2.0), pixel_point(900, -40, 3.0), pixel_point(-40, 700, 4.0)], np.float32)
    for h, w in ((1, 61), (37, 1), (9, 17)):
        want = N.rasterize(one, [[0, 1, 2]], IDENTITY[None], h, w, FOCAL)
        assert (want[1] >= 0).sum() > 0
        assert_equal_everywhere(gpu(cuda, one, [[0, 1, 2]], IDENTITY[None], h=h, w=w), want, f'one triangle over {h} x {w}')


def test_dropped_faces_and_bad_indices(cuda):
    v = np.array([[-1, 1, -3], [1, 1, -3], [0, -1, -3], [-1, 1, 3], [1, 1, 3], [0, -1, 3], [0, -1, 0.5], [3000, 1, -3], [0, 1, -3],
                  [np.nan, 0, -3], [np.inf, 0, -3]], np.float32)
    # behind the camera; straddling z = near; beyond the guard band; zero area; a NaN and an infinite vertex; and one that stays
    f = np.array([[3, 5, 4], [0, 6, 1], [0, 2, 7], [0, 8, 1], [0, 2, 9], [0, 2, 10], [0, 2, 1]], np.int32)
    want = N.rasterize(v, f, IDENTITY[None], H, W, FOCAL)
    assert set(np.unique(want[1])) == {-1, 6}
    assert_equal_everywhere(gpu(cuda, v, f, IDENTITY[None]), want, 'dropped faces')
    assert_equal_everywhere(gpu(cuda, v, f[:6], IDENTITY[None]), N.rasterize(v, f[:6], IDENTITY[None], H, W, FOCAL), 'only dropped faces')
    for bad in ([0, 1, len(v)], [0, -1, 2], [2 ** 31 - 1, 0, 1]):
        with pytest.raises(ValueError, match='face index'):
            gpu(cuda, v, np.concatenate([f, [bad]]), IDENTITY[None])
    with pytest.raises(ValueError, match='face index'):
        gpu(cuda, np.zeros((0, 3), np.float32), f, IDENTITY[None])


def test_smallest_sizes(cuda):
    v, f, col = sphere()
    poses = sphere_poses()
    want = N.rasterize(v, f, poses[:1], 1, 1, FOCAL, colors=col)
    assert want[1][0, 0, 0] >= 0
    assert_equal_everywhere(gpu(cuda, v, f, poses[:1], colors=col, h=1, w=1), want, 'H = W = 1')
    disp, face, rgb = gpu(cuda, v, f, np.zeros((0, 3, 4), np.float32), colors=col)                      # V = 0
    assert disp.shape == (0, H, W) and face.shape == (0, H, W) and rgb.shape == (0, H, W, 3)
    e3 = np.zeros((0, 3), np.float32)
    for vv, ff, cc in ((v, e3, col), (e3, e3, e3.astype(np.uint8)), (v, e3, None)):                     # F = 0; Nv = 0
        disp, face, rgb = gpu(cuda, vv, ff, poses, colors=cc)
        assert torch.all(disp == 0) and torch.all(face == -1) and (rgb is None or torch.all(rgb == 0))


def test_overlap_and_permutation(cuda):
    v = np.array([[-2, 1.5, -4], [2, 1.5, -4], [0, -1.5, -4], [-.3, .3, -2], [.3, .3, -2], [0, -.3, -2], [-1, 1, -6], [1, 1, -6],
                  [0, -1, -6], [-2, 1.5, -4], [2, 1.5, -4], [0, -1.5, -4]], np.float32)
    f = np.array([[0, 2, 1], [3, 5, 4], [6, 8, 7], [9, 11, 10]], np.int32)             # the last coincides with the first
    base = gpu(cuda, v, f, IDENTITY[None])
    assert_equal_everywhere(base, N.rasterize(v, f, IDENTITY[None], H, W, FOCAL), 'overlap')
    b_disp, b_face = base[0].cpu().numpy(), base[1].cpu().numpy()
    assert set(np.unique(b_face)) == {-1, 0, 1}             # the coincident twin loses to the lower index, the far one is hidden
    for perm in ([3, 2, 1, 0], [1, 3, 0, 2]):
        got = gpu(cuda, v, f[perm], IDENTITY[None])
        assert_equal_everywhere(got, N.rasterize(v, f[perm], IDENTITY[None], H, W, FOCAL), f'overlap, faces {perm}')
        assert np.array_equal(got[0].cpu().numpy().view(np.uint32), b_disp.view(np.uint32))
        g_face = got[1].cpu().numpy()
        hit = g_face >= 0
        back = np.asarray(perm)[g_face[hit]]                # the original index of the winner: 0 and 3 are the same triangle
        assert np.array_equal(hit, b_face >= 0) and np.array_equal(np.where(back == 3, 0, back), b_face[hit])


def test_repetition_while_the_device_is_busy(cuda):
    v, f, col, _ = large_and_tiny()
    sv, sf, scol = sphere()
    poses = np.stack([IDENTITY, Wn.pose((0., 0., .02), (.05, -.03, .1))])

    def everything():
        return gpu(cuda, v, f, poses, 'none', col) + gpu(cuda, sv, sf, sphere_poses(), 'back', scol)

    first, second = everything(), everything()
    side = torch.cuda.Stream(device=cuda)
    a = torch.randn(2048, 2048, device=cuda)
    with torch.cuda.stream(side):
        for _ in range(20):
            a = torch.tanh(a @ a * 1e-3)
    third = everything()
    side.synchronize()
    for x, y, z in zip(first, second, third):
        assert torch.equal(x.view(torch.uint8), y.view(torch.uint8)) and torch.equal(x.view(torch.uint8), z.view(torch.uint8))


def test_fragment_counters(cuda):
    v, f, col = sphere()
    out = gpu(cuda, v, f, sphere_poses(), 'none', None, stats=True)
    fragments, sent = (int(x) for x in out[3].cpu())
    frags = sum(int(N.rasterize_view(v, f, P, H, W, FOCAL)['fragments'].sum()) for P in sphere_poses())
    assert fragments == frags == 2 * 481 + 2 * 450 + 3072   # the watertight counts of tests/test_raster_cpu.py
    assert 481 + 450 + 3072 <= sent <= fragments           # every covered pixel took at least its first fragment's atomic
    assert_equal_everywhere(out, reference('sphere', v, f, sphere_poses(), 'none', None), 'the counting variant')


def test_render_views_visible_faces_keep_faces(cuda):
    v, f, col = sphere()
    m = mesh.Mesh(dev(v, cuda), dev(f, cuda), dev(np.zeros_like(v), cuda), dev(col, cuda))
    hwf = (H, W, FOCAL)
    pose = sphere_poses()[1:2]
    want = reference('sphere_view1', v, f, pose, 'none', col)
    got = mesh.render_views(m, hwf, dev(pose, cuda))
    assert_equal_everywhere(got, want, 'mesh.render_views')
    assert mesh.render_views(m, hwf, dev(pose, cuda), colors=False)[2] is None
    assert mesh.render_views(mesh.Mesh(m.verts, m.faces, None, None), hwf, pose)[2] is None               # poses from numpy
    ref = N.rasterize_view(v, f, pose[0], H, W, FOCAL)
    winners = np.unique(ref['face'][ref['face'] >= 0])
    seen = mesh.visible_faces(m, hwf, dev(pose, cuda))
    assert seen.dtype == torch.bool and seen.shape == (len(f),)
    assert np.array_equal(np.nonzero(seen.cpu().numpy())[0], winners)
    assert np.all(ref['front'][winners]) and 100 < len(winners) < ref['front'].sum()                   # seen from outside: front faces only
    three = mesh.visible_faces(m, hwf, dev(sphere_poses(), cuda), chunk=2)                            # more views see more
    assert torch.all(three[seen]) and int(three.sum()) > int(seen.sum())
    kept = mesh.keep_faces(m, seen)
    rv, rf, rn, rc = N.keep_faces(v, f, seen.cpu().numpy(), np.zeros_like(v), col)
    assert np.array_equal(kept.verts.cpu().numpy(), rv) and np.array_equal(kept.faces.cpu().numpy(), rf)
    assert np.array_equal(kept.colors.cpu().numpy(), rc) and kept.normals.shape == kept.verts.shape
    assert kept.faces.shape[0] == len(winners) < len(f) and kept.verts.shape[0] < len(v)
    again = mesh.render_views(kept, hwf, dev(pose, cuda))
    assert torch.equal(again[0].view(torch.int32), got[0].view(torch.int32)) and torch.equal(again[2], got[2])
    assert np.array_equal(winners[again[1][0].cpu().numpy()[ref['face'] >= 0]], ref['face'][ref['face'] >= 0])


def test_mesh_depth_metrics_of_a_mesh_against_its_own_render(cuda):
    v, f, col = sphere()
    m = mesh.Mesh(dev(v, cuda), dev(f, cuda), None, None)
    poses = dev(sphere_poses()[:2], cuda)
    disp = mesh.render_views(m, (H, W, FOCAL), poses)[0]
    rep = evaluate.mesh_depth_metrics(m, (H, W, FOCAL), poses, disp)
    assert rep['views'] == 2 and rep['per_view']['coverage'] == [481 / 3072, 450 / 3072]
    assert rep['per_view']['depth_l1'] == [0.0, 0.0] and rep['per_view']['depth_l2'] == [0.0, 0.0]
    masks = torch.zeros((2, H, W), dtype=torch.bool, device=cuda)
    masks[0, :, :W // 2] = True                             # the left half of view 0; nothing of view 1
    off = disp + 0.25 * masks
    rep = evaluate.mesh_depth_metrics(m, (H, W, FOCAL), poses, off, masks=masks)
    left = int((disp[0, :, :W // 2] > 0).sum())
    assert rep['per_view']['coverage_masked'] == [left / (H * W // 2), None]
    assert rep['per_view']['depth_l1_masked'][1] is None and rep['per_view']['depth_l2_masked'][1] is None
    assert rep['per_view']['depth_l1_masked'][0] == pytest.approx(0.25, abs=1e-6)          # fp32 sums of disp + 0.25 - disp
    assert rep['per_view']['depth_l2_masked'][0] == pytest.approx(0.0625, abs=1e-6)
    assert abs(rep['per_view']['depth_l1'][0] - 0.25 * left / 481) < 1e-6 and rep['per_view']['depth_l1'][1] == 0.0
    with pytest.raises(ValueError, match='disparities'):
        evaluate.mesh_depth_metrics(m, (H, W, FOCAL), poses, disp[:1])


def test_tsdf_mesh_of_the_tiny_model_renders(cuda):
    """mesh.extract_mesh_tsdf of the seeded 8 x 256 pair (the construction of tests/test_tsdf.py, written again) seen again
    through its own cameras: the mesh covers part of every view."""
    from oracle.weights import seeded_state_dict
    _, te, _, _, _ = run.create_nerf(bench.make_args(), device=cuda)
    sel = torch.from_numpy(np.random.RandomState(99).randint(0, bench.H * bench.W, 2000)).to(cuda)
    rows = ops.ray_rows_from_pose(bench.orbit_pose(0, cuda), bench.H, bench.W, bench.FOCAL, bench.NEAR, bench.FAR, sel=sel)
    z = ops.stratified_z(rows, 64, True)
    pts = (rows[:, None, 0:3] + rows[:, None, 3:6] * z[:, :, None]).reshape(-1, 3)
    dirs = rows[:, None, 8:11].expand(-1, 64, -1).reshape(-1, 3).contiguous()
    for net, seed in ((te['network_fn'], 1), (te['network_fine'], 2)):
        net.load_state_dict({k: torch.from_numpy(w) for k, w in seeded_state_dict(seed).items()})
        with torch.no_grad():
            sigma = net.query_points(pts, dirs)[:, 3]
            scale = 4.0 / float(sigma.std())
            net.alpha_linear.bias.copy_((net.alpha_linear.bias - sigma.median()) * scale)
            net.alpha_linear.weight.mul_(scale)
        net.invalidate_packed()
    h, w = 12, 16
    hwf = (h, w, bench.FOCAL * w / bench.W)
    poses = torch.stack([bench.orbit_pose(k, cuda)[:3, :4] for k in (0, 2, 58)]).contiguous()
    lo, hi = mesh.frustum_bounds(poses, hwf, bench.NEAR, bench.FAR)
    m = mesh.extract_mesh_tsdf(te, hwf, poses, bench.NEAR, bench.FAR, lo, hi, resolution=9)
    assert m.faces.shape[0] > 0
    disp, face, rgb = mesh.render_views(m, hwf, poses)
    cover = [float((face[i] >= 0).float().mean()) for i in range(3)]
    print(f'tiny model: {m.faces.shape[0]} triangles, coverage per view {cover}')
    assert all(c > 0 for c in cover) and rgb.shape == (3, h, w, 3)
    assert int(mesh.visible_faces(m, hwf, poses).sum()) > 0


def test_extract_mesh_tool_drops_unseen_faces(cuda, tmp_path, capsys):
    """tools/extract_mesh.py --tsdf --fixture --drop-unseen on a field of two training iterations (a second run of the tool
    would train another field, so the file is checked against the counts the tool prints, not against a run without the flag)."""
    import re
    from tools import extract_mesh as T
    seen = str(tmp_path / 'seen.ply')
    assert T.main(['--tsdf', '--fixture', '--iters', '2', '--view-step', '10', '--resolution', '24', '--out', seen, '--drop-unseen']) == 0
    text = capsys.readouterr().out
    m = re.search(r'visible from 3 views of \d+ x \d+: (\d+) triangles, (\d+) vertices -> (\d+) triangles, (\d+) vertices', text)
    assert m and 'visibility' in text
    f0, v0, f1, v1 = (int(x) for x in m.groups())
    assert 0 < f1 <= f0 and 0 < v1 <= v0
    head, sv, sf = M.read_ply(seen)
    assert len(sf) == f1 and len(sv) == v1 and f'element vertex {v1}' in head and f'element face {f1}' in head
    assert np.array_equal(np.unique(sf), np.arange(v1))    # every vertex is referenced
    with pytest.raises(SystemExit):                        # without --tsdf the cameras have to come from --datadir
        T.main([str(tmp_path / 'none.tar'), '--out', seen, '--drop-unseen'])


def test_operand_checks(cuda):
    v, f, col = sphere()
    tv, tf, tp, tc = dev(v, cuda), dev(f, cuda), dev(sphere_poses(), cuda), dev(col, cuda)
    call = lambda a=tv, b=tf, p=tp, h=H, w=W, focal=FOCAL, **kw: ops.mesh_rasterize(a, b, p, h, w, focal, **kw)
    with pytest.raises(ValueError, match='no CPU path'):
        call(tv.cpu(), tf.cpu(), tp.cpu())
    with pytest.raises(ValueError, match='no CPU path'):
        call(p=tp.cpu())
    with pytest.raises(ValueError, match='must be torch.float32'):
        call(tv.double())
    with pytest.raises(ValueError, match='must be torch.int32'):
        call(b=tf.long())
    with pytest.raises(ValueError, match='must be torch.float32'):
        call(p=tp.double())
    with pytest.raises(ValueError, match='must be torch.uint8'):
        call(colors=tc.float())
    with pytest.raises(ValueError, match='colors'):
        call(colors=tc[:5].contiguous())
    with pytest.raises(ValueError, match=r'\[V, 3\]'):
        call(tv.reshape(-1))
    with pytest.raises(ValueError, match=r'\[F, 3\]'):
        call(b=tf[:, :2].contiguous())
    with pytest.raises(ValueError, match=r'\[N, 3, 4\]'):
        call(p=tp[:, :, :3].contiguous())
    with pytest.raises(ValueError, match='contiguous'):
        call(b=tf.t().contiguous().t())
    with pytest.raises(ValueError, match='contiguous'):
        call(p=tp.transpose(1, 2).contiguous().transpose(1, 2))
    with pytest.raises(ValueError, match='tensor on the GPU'):
        call(v)
    for h, w in ((0, W), (H, 0), (16385, W), (H, 16385), (4.5, W)):
        with pytest.raises(ValueError, match='H and W'):
            call(h=h, w=w)
    for bad in (0.0, -1.0, float('nan'), float('inf')):
        with pytest.raises(ValueError, match='finite and > 0'):
            call(focal=bad)
        with pytest.raises(ValueError, match='finite and > 0'):
            call(near=bad)
    with pytest.raises(ValueError, match='cull'):
        call(cull='front')


def test_abi_refuses_before_any_device_call(cuda):
    lib = _lib.load()
    buf = torch.zeros(1024, device=cuda, dtype=torch.int32)
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(buf.data_ptr())
    st = _lib.stream()
    big = 2 ** 31
    nan, inf = float('nan'), float('inf')
    # (verts, faces, Nv, F, poses, V, H, W, focal, near, cull, keys, flag, stats)
    good = [one, one, 3, 1, one, 1, 4, 4, 1.0, 1e-3, 0, one, one, null]
    changes = [(0, null), (1, null), (4, null), (11, null), (12, null), (2, -1), (3, -1), (5, -1), (2, big), (3, big // 3 + 1), (5, big),
               (6, 0), (6, 16385), (6, -4), (7, 0), (7, 16385), (8, 0.0), (8, -1.0), (8, nan), (8, inf), (9, 0.0), (9, -1e-3), (9, nan),
               (9, inf), (10, 2), (10, -1)]
    for k, value in changes:
        args = list(good)
        args[k] = value
        assert lib.mvip_raster_fragments(*args, st) == -1, (k, value)
    # (keys, verts, faces, colors, Nv, F, poses, V, H, W, focal, near, disp, face, rgb)
    good = [one, one, one, one, 3, 1, one, 1, 4, 4, 1.0, 1e-3, one, one, one]
    changes = [(0, null), (1, null), (2, null), (6, null), (12, null), (13, null), (3, null), (4, -1), (5, -1), (7, -1), (4, big),
               (5, big // 3 + 1), (7, big), (8, 0), (8, 16385), (9, 0), (9, 16385), (10, 0.0), (10, nan), (10, inf), (11, 0.0), (11, nan),
               (11, inf)]
    for k, value in changes:
        args = list(good)
        args[k] = value
        assert lib.mvip_raster_resolve(*args, st) == -1, (k, value)
    torch.cuda.synchronize()
    assert int(buf.abs().sum()) == 0                        # nothing was written
