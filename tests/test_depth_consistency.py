"""Cross-view depth consistency on the GPU (csrc/depth_consistency.hip) against the restatement
tests/depth_consistency_numpy.py: both counts EXACTLY (the kernel and the restatement evaluate the same fp64 expressions in the
same association), order independence, repetition, masks and bad disparities; prepare.consistency_mask and the filters of
mesh.extract_mesh_tsdf."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import depth_consistency_numpy as R                      # noqa: E402
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench                                             # noqa: E402
from mvip_nerf_amd import mesh, ops, prepare, run        # noqa: E402

pytestmark = pytest.mark.gpu


def gpu(dev, disp, poses, focal, masks=None, tol=0.05):
    m = None if masks is None else torch.from_numpy(np.ascontiguousarray(masks)).to(dev)
    a, v = ops.depth_consistency(torch.from_numpy(np.ascontiguousarray(disp, np.float32)).to(dev),
                                 torch.from_numpy(np.ascontiguousarray(poses, np.float32)).to(dev), focal, masks=m, tol=tol)
    assert a.dtype == torch.int32 and v.dtype == torch.int32 and tuple(a.shape) == tuple(v.shape) == tuple(disp.shape)
    return a.cpu().numpy(), v.cpu().numpy()


def check(dev, disp, poses, focal, masks=None, tol=0.05):
    want = R.consistency(disp, poses, focal, tol, masks)
    got = gpu(dev, disp, poses, focal, masks, tol)
    assert np.array_equal(got[0], want[0]), np.argwhere(got[0] != want[0])[:5]
    assert np.array_equal(got[1], want[1]), np.argwhere(got[1] != want[1])[:5]
    return got


@pytest.fixture(scope='module')
def scene():
    return R.trial_scene3()


@pytest.mark.parametrize('floater', [False, True])
def test_trial_scene(floater, scene, cuda):
    case = R.with_floater(scene) if floater else scene
    agree, violated = check(cuda, case['disp'], case['poses'], case['focal'])
    assert agree.max() == 2 and (agree > 0).mean() > 0.8
    if floater:
        assert (agree[0][R.FLOATER] == 0).all() and (violated[0][R.FLOATER] >= 1).all()
    for tol in (0.005, 0.3):
        check(cuda, case['disp'], case['poses'], case['focal'], tol=tol)


def test_one_plane_every_projection_agrees(cuda):
    c = R.homography_case3()
    agree, violated = check(cuda, c['disp'], c['poses'], c['focal'])
    H, W, f = c['H'], c['W'], c['focal']
    assert not violated.any()
    import warp_numpy as wn
    for n in range(3):
        o, d = wn.pixel_rays(c['poses'][n], H, W, f)
        pts = o + (1.0 / c['disp'][n].astype(np.float64))[..., None] * d
        lands = np.zeros((H, W), np.int32)
        clear = np.ones((H, W), bool)                        # no projection within 1e-6 of the image border
        for s in range(3):
            if s != n:
                ts, u, v = R.project(pts, c['poses'][s], f, H, W)
                lands += (ts > 0) & (u >= 0) & (u <= W - 1) & (v >= 0) & (v <= H - 1)
                clear &= (np.abs(u) > 1e-6) & (np.abs(u - (W - 1)) > 1e-6) & (np.abs(v) > 1e-6) & (np.abs(v - (H - 1)) > 1e-6)
        assert clear.mean() > 0.99 and np.array_equal(agree[n][clear], lands[clear])
    assert agree.max() == 2


def test_bad_disparities_masks_and_few_views(scene, cuda):
    d = scene['disp'].copy()
    rs = np.random.RandomState(3)
    idx = rs.rand(*d.shape) < 0.05
    d[idx] = rs.choice(np.array([np.nan, np.inf, -np.inf, 0.0, -0.3], np.float32), int(idx.sum()))
    agree, violated = check(cuda, d, scene['poses'], scene['focal'])
    assert not agree[idx].any() and not violated[idx].any()
    m = rs.rand(*d.shape) < 0.9
    a2, v2 = check(cuda, scene['disp'], scene['poses'], scene['focal'], masks=m)
    assert not a2[~m].any() and not v2[~m].any()
    z = np.where(m, scene['disp'], np.float32(0))
    assert np.array_equal(a2, gpu(cuda, z, scene['poses'], scene['focal'])[0])           # a masked pixel is a zeroed pixel
    for V in (0, 1, 2):
        a, v = check(cuda, scene['disp'][:V], scene['poses'][:V], scene['focal'])
        assert a.shape == (V, scene['H'], scene['W']) and (V == 2 or (not a.any() and not v.any()))


def test_two_by_two_image(cuda):
    import warp_numpy as wn
    poses = np.stack([wn.pose((0.0, 0.0, 0.0), (0.0, 0.0, 0.0)), wn.pose((0.0, 0.01, 0.0), (0.02, 0.0, 0.0)), wn.pose((0.01, 0.0, 0.0), (0.0, -0.02, 0.0))])
    disp = np.stack([wn.plane_disparity(p, 2, 2, 2.0, (0.0, 0.0, 1.0), -3.0).astype(np.float32) for p in poses])
    disp[2, 1, 1] *= np.float32(2.0)                         # a floater in the corner
    agree, violated = check(cuda, disp, poses, 2.0)
    assert agree.any()


def test_counts_do_not_depend_on_the_order_of_the_other_views_and_a_call_equals_its_repetition(scene, cuda):
    case = R.with_floater(scene)
    first = gpu(cuda, case['disp'], case['poses'], case['focal'])
    again = gpu(cuda, case['disp'], case['poses'], case['focal'])
    assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1])
    perm = [0, 2, 1]
    a, v = gpu(cuda, case['disp'][perm], case['poses'][perm], case['focal'])
    assert np.array_equal(a[0], first[0][0]) and np.array_equal(v[0], first[1][0])
    assert np.array_equal(a[1], first[0][2]) and np.array_equal(v[2], first[1][1])


def test_consistency_mask(scene, cuda):
    case = R.with_floater(scene)
    d, p = torch.from_numpy(case['disp']).to(cuda), torch.from_numpy(case['poses']).to(cuda)
    a, v = ops.depth_consistency(d, p, case['focal'])
    keep = prepare.consistency_mask(d, p, case['focal'])
    assert keep.dtype == torch.bool and torch.equal(keep, (a >= 1) & (v <= 0))
    assert not keep[0][R.FLOATER].any()
    assert torch.equal(prepare.consistency_mask(d, p, case['focal'], min_agree=2, max_violated=1), (a >= 2) & (v <= 1))
    assert prepare.consistency_mask(d, p, case['focal'], min_agree=0, max_violated=2 ** 31 - 1).all()


# ---- the filters of mesh.extract_mesh_tsdf ------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def mlp(cuda):
    """The seeded 8 x 256 pair with a density head that renders something (the construction of tests/test_tsdf.py, written
    again): alpha_linear rescaled to sigma' = 4 (sigma - median) / std over the camera's sample points."""
    from oracle.weights import seeded_state_dict
    _, te, _, _, _ = run.create_nerf(bench.make_args(), device=cuda)
    sel = torch.from_numpy(np.random.RandomState(99).randint(0, bench.H * bench.W, 2000)).to(cuda)
    rows = ops.ray_rows_from_pose(bench.orbit_pose(0, cuda), bench.H, bench.W, bench.FOCAL, bench.NEAR, bench.FAR, sel=sel)
    z = ops.stratified_z(rows, 64, True)
    pts = (rows[:, None, 0:3] + rows[:, None, 3:6] * z[:, :, None]).reshape(-1, 3)
    dirs = rows[:, None, 8:11].expand(-1, 64, -1).reshape(-1, 3).contiguous()
    for net, seed in ((te['network_fn'], 1), (te['network_fine'], 2)):
        net.load_state_dict({k: torch.from_numpy(v) for k, v in seeded_state_dict(seed).items()})
        with torch.no_grad():
            sigma = net.query_points(pts, dirs)[:, 3]
            scale = 4.0 / float(sigma.std())
            net.alpha_linear.bias.copy_((net.alpha_linear.bias - sigma.median()) * scale)
            net.alpha_linear.weight.mul_(scale)
        net.invalidate_packed()
    return te


def test_extract_mesh_tsdf_filters_are_masks_handed_to_fuse_depths(mlp, cuda):
    H, W = 24, 32
    hwf = (H, W, bench.FOCAL * W / bench.W)
    poses = torch.stack([bench.orbit_pose(k, cuda)[:3, :4] for k in (0, 2, 58)]).contiguous()
    lo, hi = mesh.frustum_bounds(poses, hwf, bench.NEAR, bench.FAR)
    args = (mlp, hwf, poses, bench.NEAR, bench.FAR, lo, hi)
    same = lambda a, b: torch.equal(a.verts.view(torch.int32), b.verts.view(torch.int32)) and torch.equal(a.faces, b.faces)
    # the defaults: today's call
    expected = prepare.render_disparities(mlp, hwf, poses, bench.NEAR, bench.FAR)
    today = mesh.fuse_depths(expected, poses, hwf[2], lo, hi, resolution=32)
    assert same(mesh.extract_mesh_tsdf(*args, resolution=32, colors=False), today)
    assert same(mesh.extract_mesh_tsdf(*args, resolution=32, colors=False, depth='expected', max_spread=None, min_agree=None, max_violated=None), today)
    assert today.faces.shape[0] > 0
    # median + spread + agreement, by hand
    q = prepare.render_depth_quantiles(mlp, hwf, poses, bench.NEAR, bench.FAR, (0.16, 0.5, 0.84))
    median = (1.0 / q[..., 1]).contiguous()
    assert torch.equal(median.view(torch.int32), prepare.render_disparities(mlp, hwf, poses, bench.NEAR, bench.FAR, kind='median').view(torch.int32))
    user = torch.ones((3, H, W), dtype=torch.bool, device=cuda)
    user[:, :2] = False
    r = float(np.median(((q[..., 2] - q[..., 0]) / q[..., 1])[torch.isfinite(q).all(-1)].cpu().numpy()))      # keeps about half
    spread = torch.isfinite(q).all(-1) & ((q[..., 2] - q[..., 0]) / q[..., 1] <= r)
    cons = prepare.consistency_mask(median, poses, hwf[2], min_agree=1, max_violated=2 ** 31 - 1)
    assert 0.2 < spread.float().mean() < 0.8
    want = mesh.fuse_depths(median, poses, hwf[2], lo, hi, resolution=32, masks=user & spread & cons)
    got = mesh.extract_mesh_tsdf(*args, resolution=32, colors=False, masks=user, depth='median', max_spread=r, min_agree=1)
    assert same(got, want)
    assert same(mesh.extract_mesh_tsdf(*args, resolution=32, colors=False, depth='median'), mesh.fuse_depths(median, poses, hwf[2], lo, hi, resolution=32))
    assert not same(got, today)
    with pytest.raises(ValueError, match='kind'):
        mesh.extract_mesh_tsdf(*args, resolution=32, depth='mode')
