"""TSDF depth-map fusion (csrc/tsdf.hip) and marching cubes on observed cells (mvip_mcubes_count_valid) on the GPU, against the
numpy restatement tests/tsdf_numpy.py: counts equal and |tsdf - fp64| <= 4 e32 + 2^-22 off the excluded points (e32: the fp32
restatement's own distance from the fp64 one, per case -- the rule of tests/test_warp.py), bit-equal repetition, masks and bad
disparities; masked marching cubes against its restatement; mesh.fuse_depths / extract_mesh_tsdf / tools/extract_mesh.py --tsdf."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mc_numpy as M                                     # noqa: E402
import tsdf_numpy as R                                   # noqa: E402
from warp_numpy import pose                              # noqa: E402
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench                                             # noqa: E402
from mvip_nerf_amd import mesh, ops, prepare, run        # noqa: E402

pytestmark = pytest.mark.gpu

MAX_EXCLUDED = 0.01
FLOOR = 2.0 ** -22


def gpu_fuse(dev, disp, poses, focal, lo, hi, res, trunc, masks=None):
    m = None if masks is None else torch.from_numpy(np.ascontiguousarray(masks)).to(dev)
    t, c = ops.tsdf_fuse(torch.from_numpy(np.ascontiguousarray(disp, np.float32)).to(dev),
                         torch.from_numpy(np.ascontiguousarray(poses, np.float32)).to(dev), focal, lo, hi, res, trunc, masks=m)
    assert t.dtype == torch.float32 and c.dtype == torch.int32 and t.shape == c.shape == tuple(R.resolution3(res))
    return t.cpu().numpy(), c.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def small_case():
    """The trial scene on a 2 x 2 x 2 lattice that straddles the box face."""
    c = R.trial_case()
    return dict(c, bound_min=(-0.31, -0.22, -3.13), bound_max=(0.43, 0.33, -2.27), resolution=(2, 2, 2))


def one_pixel_case():
    """H = W = 1: two cameras that see one surface element each; a 5 x 4 x 6 lattice along their axes."""
    poses = np.stack([pose((0.01, -0.02, 0.015), (0.003, 0.007, 0.011)), pose((-0.012, 0.017, -0.02), (-0.004, 0.006, -0.013))])
    disp = np.array([[[1 / 3.0]], [[1 / 2.9]]], np.float32)
    return dict(disp=disp, poses=poses, focal=2.0, bound_min=(-0.63, -0.52, -3.77), bound_max=(0.58, 0.61, -2.21), resolution=(5, 4, 6),
                trunc=0.5)


def behind_case():
    """The trial scene with a fourth camera that looks the other way: the whole lattice lies behind it."""
    c = R.trial_case()
    back = pose((0.02, np.pi + 0.03, 0.01), (0.011, 0.023, 0.017))
    return dict(c, poses=np.concatenate([c['poses'], back[None]]), disp=np.concatenate([c['disp'], c['disp'][:1]]))


FUSION_CASES = {'trial': R.trial_case, 'plane17': lambda: R.plane_case(R.PLANE_LATTICES[0]), 'plane33': lambda: R.plane_case(R.PLANE_LATTICES[1]),
                'lattice2': small_case, 'one_pixel': one_pixel_case, 'behind': behind_case}
_YARD = {}


def yard(name):
    if name not in _YARD:
        case = FUSION_CASES[name]()
        _YARD[name] = (case, R.yardstick(*R.args_of(case)))
    return _YARD[name]


@pytest.mark.parametrize('name', sorted(FUSION_CASES))
def test_fusion_matches_the_restatement(name, cuda):
    case, y = yard(name)
    V = case['disp'].shape[0]
    t, c = gpu_fuse(cuda, *R.args_of(case))
    keep = ~y['excluded']
    err = float(np.abs(t.astype(np.float64) - y['tsdf'])[keep].max())
    tol = 4 * y['e32'] + FLOOR
    print(f'{name}: excluded {y["excluded_share"]:.4%}, e32 {y["e32"]:.3g}, |gpu - fp64| {err:.3g} (bound {tol:.3g}), '
          f'counts differing {int((c != y["count"])[keep].sum())}, observed {float((c > 0).mean()):.3f}')
    assert y['excluded_share'] <= MAX_EXCLUDED
    assert np.array_equal(c[keep], y['count'][keep])
    assert err <= tol
    assert np.all((t >= -1) & (t <= 1)) and np.all((c >= 0) & (c <= V)) and np.all(t[c == 0] == 1)      # excluded points included
    t2, c2 = gpu_fuse(cuda, *R.args_of(case))
    assert np.array_equal(bits(t), bits(t2)) and np.array_equal(c, c2)
    if name == 'behind':
        t3, c3 = gpu_fuse(cuda, case['disp'][:3], case['poses'][:3], *R.args_of(case)[2:])
        assert np.array_equal(bits(t), bits(t3)) and np.array_equal(c, c3)
    if name in ('trial', 'lattice2', 'one_pixel'):
        assert (c > 0).any()


def test_no_views_means_unobserved_everywhere(cuda):
    t, c = gpu_fuse(cuda, np.zeros((0, 48, 64), np.float32), np.zeros((0, 3, 4), np.float32), 60.0, (-1, -1, -4), (1, 1, -1), (5, 6, 7), 0.4)
    assert np.all(t == 1) and np.all(c == 0)


def test_masked_view_equals_the_call_without_it(cuda):
    case = R.trial_case()
    args = R.args_of(case)
    V, H, W = case['disp'].shape
    m = np.ones((V, H, W), bool)
    m[1] = False
    t1, c1 = gpu_fuse(cuda, *args, masks=m)
    t2, c2 = gpu_fuse(cuda, case['disp'][[0, 2]], case['poses'][[0, 2]], *args[2:])
    assert np.array_equal(bits(t1), bits(t2)) and np.array_equal(c1, c2)
    t0, c0 = gpu_fuse(cuda, *args)
    assert (c1 < c0).any() and (c1 <= c0).all()
    ta, ca = gpu_fuse(cuda, *args, masks=np.ones((V, H, W), bool))
    assert np.array_equal(bits(ta), bits(t0)) and np.array_equal(ca, c0)


@pytest.mark.parametrize('bad', [np.nan, np.inf, 0.0, -0.5], ids=['nan', 'inf', 'zero', 'negative'])
def test_a_bad_disparity_unsees_its_pixel_and_nothing_else(bad, cuda):
    case = R.trial_case()
    args = R.args_of(case)
    V, H, W = case['disp'].shape
    py, px = R.hit_pixel(case, 0)
    d = case['disp'].copy()
    d[0, py, px] = bad
    mm = np.ones((V, H, W), bool)
    mm[0, py, px] = False
    tb, cb = gpu_fuse(cuda, d, *args[1:])
    tm, cm = gpu_fuse(cuda, *args, masks=mm)
    t0, c0 = gpu_fuse(cuda, *args)
    assert np.array_equal(bits(tb), bits(tm)) and np.array_equal(cb, cm)
    assert (cb < c0).any() and (cb <= c0).all()


def test_tsdf_fuse_argument_errors(cuda):
    case = R.trial_case()
    d, p = torch.from_numpy(case['disp']).to(cuda), torch.from_numpy(case['poses']).to(cuda)
    lo, hi, res = case['bound_min'], case['bound_max'], case['resolution']
    for kw in (dict(resolution=(1, 5, 5)), dict(resolution=769), dict(trunc=0.0), dict(trunc=float('nan')), dict(focal=0.0),
               dict(bound_min=(1.3, -0.9, -4.4)), dict(poses=p[:2]), dict(masks=torch.ones((3, 48, 63), dtype=torch.bool, device=cuda)),
               dict(disp=d.cpu()), dict(disp=d.double())):
        a = dict(disp=d, poses=p, focal=60.0, bound_min=lo, bound_max=hi, resolution=res, trunc=0.4, masks=None)
        a.update(kw)
        with pytest.raises(ValueError):
            ops.tsdf_fuse(**a)


# ---- marching cubes on observed cells -------------------------------------------------------------------------------------------------

LO, HI = (-1.0, -0.5, 0.25), (1.5, 0.75, 2.0)


def gpu_mc(dev, g, valid):
    v = None if valid is None else torch.from_numpy(valid).to(dev)
    return tuple(x.cpu().numpy() for x in mesh.marching_cubes(torch.from_numpy(g).to(dev), 1.0, LO, HI, valid=v))


def random_grid(seed=11, shape=(13, 9, 21)):
    rs = np.random.RandomState(seed)
    return (rs.rand(*shape) * 2).astype(np.float32), rs.rand(*shape) < 0.7


def test_all_valid_is_the_unmasked_path_bit_for_bit(cuda):
    g, _ = random_grid()
    a = gpu_mc(cuda, g, None)
    for valid in (np.ones(g.shape, bool), np.full(g.shape, 7, np.uint8)):
        b = gpu_mc(cuda, g, valid)
        assert len(a[1]) > 100
        assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(a[1], b[1]) and np.array_equal(bits(a[2]), bits(b[2]))


def test_random_validity_matches_the_restatement(cuda):
    g, valid = random_grid()
    verts, faces, normals = gpu_mc(cuda, g, valid)
    rv, rf, _ = R.marching_cubes_valid(g, valid, 1.0, LO, HI)
    full = gpu_mc(cuda, g, None)
    print(f'13 x 9 x 21, {valid.mean():.0%} valid: {len(faces)} of {len(full[1])} triangles, {len(verts)} of {len(full[0])} vertices')
    assert 0 < len(faces) < len(full[1])
    assert faces.dtype == np.int32 and np.array_equal(faces, rf)
    assert np.array_equal(bits(verts), bits(rv))
    assert np.array_equal(np.unique(faces), np.arange(len(verts)))                       # no unreferenced vertex
    assert normals.shape == verts.shape and np.isfinite(normals).all()
    again = gpu_mc(cuda, g, valid)
    assert all(np.array_equal(x, z) for x, z in zip((verts, faces, normals), again))


def test_no_valid_point_gives_an_empty_mesh(cuda):
    g, _ = random_grid()
    verts, faces, normals = mesh.marching_cubes(torch.from_numpy(g).to(cuda), 1.0, LO, HI, valid=torch.zeros(g.shape, dtype=torch.bool, device=cuda))
    assert tuple(verts.shape) == (0, 3) and tuple(faces.shape) == (0, 3) and tuple(normals.shape) == (0, 3)
    assert faces.dtype == torch.int32 and verts.is_cuda


def test_non_finite_values_matter_at_valid_points_only(cuda):
    g, valid = random_grid()
    i, j, k = (int(x[0]) for x in np.nonzero(~valid))
    g2 = g.copy()
    g2[i, j, k] = np.nan
    verts, faces, _ = gpu_mc(cuda, g2, valid)
    rv, rf, _ = R.marching_cubes_valid(g, valid, 1.0, LO, HI)
    assert np.array_equal(faces, rf) and np.array_equal(bits(verts), bits(rv))
    i, j, k = (int(x[0]) for x in np.nonzero(valid))
    for bad in (np.nan, np.inf):
        g3 = g.copy()
        g3[i, j, k] = bad
        with pytest.raises(ValueError, match='non-finite'):
            gpu_mc(cuda, g3, valid)
    with pytest.raises(ValueError, match='valid'):
        gpu_mc(cuda, g, valid[:-1])
    with pytest.raises(ValueError, match='valid'):
        mesh.marching_cubes(torch.from_numpy(g).to(cuda), 1.0, LO, HI, valid=torch.ones(g.shape, device=cuda))


# ---- the pipeline -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('res', R.PLANE_LATTICES, ids=['17x13x21', '33x25x41'])
def test_fuse_depths_puts_the_plane_where_it_is(res, cuda):
    case = R.plane_case(res)
    d, p = torch.from_numpy(case['disp']).to(cuda), torch.from_numpy(case['poses']).to(cuda)
    m = mesh.fuse_depths(d, p, case['focal'], case['bound_min'], case['bound_max'], resolution=res)        # trunc=None: four steps
    assert m.colors is None and m.verts.is_cuda and m.faces.dtype == torch.int32
    verts, faces, normals = m.verts.cpu().numpy(), m.faces.cpu().numpy(), m.normals.cpu().numpy()
    assert len(faces) > 100 and np.array_equal(np.unique(faces), np.arange(len(verts)))
    dist, cos = R.plane_mesh_figures(verts, normals, case)
    print(f'{res}: {len(verts)} vertices, {len(faces)} triangles, farthest {dist:.3f} of a step, smallest cosine {cos:.4f}')
    assert dist <= 0.5
    assert cos >= 0.9
    # the same mesh as the restatement's, from the kernel's own field
    t, c = ops.tsdf_fuse(d, p, case['focal'], case['bound_min'], case['bound_max'], res, case['trunc'])
    g, valid = R.mc_lattice(t.cpu().numpy(), c.cpu().numpy())
    rv, rf, _ = R.marching_cubes_valid(g, valid, 1.0, case['bound_min'], case['bound_max'])
    assert np.array_equal(faces, rf) and np.array_equal(bits(verts), bits(rv))
    one = mesh.fuse_depths(d, p, case['focal'], case['bound_min'], case['bound_max'], resolution=res, largest=1)
    assert torch.equal(one.faces, m.faces) and torch.equal(one.verts, m.verts)                             # one sheet already


@pytest.fixture(scope='module')
def mlp(cuda):
    """The seeded 8 x 256 pair with a density head that renders something (the construction of tests/test_prepare.py, written
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


def test_extract_mesh_tsdf_is_render_then_fuse(mlp, cuda):
    H, W = 12, 16
    hwf = (H, W, bench.FOCAL * W / bench.W)
    poses = torch.stack([bench.orbit_pose(k, cuda)[:3, :4] for k in (0, 2, 58)]).contiguous()
    lo, hi = mesh.frustum_bounds(poses, hwf, bench.NEAR, bench.FAR)
    m = mesh.extract_mesh_tsdf(mlp, hwf, poses, bench.NEAR, bench.FAR, lo, hi, resolution=9)
    disp = prepare.render_disparities(mlp, hwf, poses, bench.NEAR, bench.FAR)
    want = mesh.fuse_depths(disp, poses, hwf[2], lo, hi, resolution=9)
    print(f'tiny model: {m.verts.shape[0]} vertices, {m.faces.shape[0]} triangles')
    assert m.verts.shape[0] > 0 and m.faces.shape[0] > 0
    assert torch.equal(m.verts.view(torch.int32), want.verts.view(torch.int32)) and torch.equal(m.faces, want.faces)
    assert m.colors.dtype == torch.uint8 and tuple(m.colors.shape) == (m.verts.shape[0], 3)
    assert mesh.extract_mesh_tsdf(mlp, hwf, poses, bench.NEAR, bench.FAR, lo, hi, resolution=9, colors=False).colors is None
    with pytest.raises(ValueError, match='NDC'):
        mesh.extract_mesh_tsdf(dict(mlp, ndc=True), hwf, poses, bench.NEAR, bench.FAR, lo, hi, resolution=9)


def test_extract_mesh_tool_tsdf_route(cuda, tmp_path, capsys):
    from tools import extract_mesh as T
    out = str(tmp_path / 'tsdf.ply')
    assert T.main(['--tsdf', '--fixture', '--iters', '2', '--view-step', '10', '--resolution', '24', '--out', out]) == 0
    text = capsys.readouterr().out
    assert 'observed share of the lattice' in text and 'fusion' in text and 'marching cubes' in text
    head, vert, faces = M.read_ply(out)
    assert f'element vertex {len(vert)}' in head and f'element face {len(faces)}' in head
    assert f'{len(vert)} vertices, {len(faces)} triangles' in text
    if len(vert):
        assert 'red' in vert.dtype.names and faces.min() >= 0 and faces.max() < len(vert)
