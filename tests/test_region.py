"""Regions on the GPU (mvip_nerf_amd/region.py, csrc/region.hip, run.render_rays' `region` keyword): the mark / lookup /
accumulate kernels against the numpy restatement (tests/region_numpy.py), the 'region_map' of every render route against the
accumulate kernel on that call's own outputs, carve() against the masked chain written from existing ops, mask lifting and
propagation end to end on an analytic scene whose masks are derivable, and once on a trained field."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import occupancy_numpy as R                              # noqa: E402
import region_numpy as G                                 # noqa: E402

import bench                                             # noqa: E402
from mvip_nerf_amd import ops, run                       # noqa: E402
from mvip_nerf_amd.occupancy import OccupancyGrid        # noqa: E402
from mvip_nerf_amd.region import Region, propagate_masks  # noqa: E402
from mvip_nerf_amd.run_nerf_helpers import _uniforms     # noqa: E402

pytestmark = pytest.mark.gpu

# the camera of bench.orbit_pose(0) sits at (0, 0, 0.3) and looks down -z, samples at depth 1.2 .. 7.74: every ray enters
# this box and leaves it (the box of tests/test_occupancy.py)
BOX = ((-1.5, -1.2, -4.3), (1.5, 1.2, -0.7))
CELLS = (40, 33, 64)


def N(t):
    return t.detach().cpu().numpy()


def random_cells(cells, seed=7):
    return np.random.RandomState(seed).rand(*cells) < 0.5


def make_region(reg, cuda, box=BOX):
    return Region(box[0], box[1], reg.shape, torch.from_numpy(R.pack(reg)).to(cuda))


def bench_rows(cuda, B, seed=0):
    sel = torch.from_numpy(np.random.RandomState(seed).randint(0, bench.H * bench.W, B)).to(cuda)
    return ops.ray_rows_from_pose(bench.orbit_pose(0, cuda), bench.H, bench.W, bench.FOCAL, bench.NEAR, bench.FAR, sel=sel)


def points_np(rows, z):
    """The sample points in the kernels' expression, restated: fp32 product, then fp32 sum (no contraction)."""
    r, z = N(rows).astype(np.float32), N(z).astype(np.float32)
    with np.errstate(invalid='ignore', over='ignore'):
        return (r[:, None, 0:3] + (r[:, None, 3:6] * z[:, :, None]).astype(np.float32)).astype(np.float32)


def seeded_points(P, seed):
    rs = np.random.RandomState(seed)
    lo, hi = np.float32(BOX[0]), np.float32(BOX[1])
    pts = (lo + (hi - lo) * rs.uniform(-0.2, 1.2, (P, 3))).astype(np.float32)
    if P >= 2000:
        pts[:6] = [[np.nan, 0, -2], [0, np.inf, -2], [0, 0, -np.inf], lo, hi, (lo + hi) / 2]
        pts[100:1100] = (lo + (hi - lo) * (rs.randint(0, 41, (1000, 3)) / np.float32(40))).astype(np.float32)   # cell and box faces
    return pts, lo, hi


# ---- 1. mark / lookup ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('cells', [(5, 3, 7), (40, 33, 64), (64, 1, 1)])
@pytest.mark.parametrize('P', [0, 1, 10 ** 6])
def test_mark_equals_restatement(P, cells, cuda):
    pts, lo, hi = seeded_points(P, P % 1000 + cells[0])
    if P == 1:
        pts[0] = (lo + hi) / 2
    want = G.mark(pts, lo, hi, cells)
    t = torch.from_numpy(pts).to(cuda)
    r = Region.from_points(t, lo, hi, cells, dilate=0)
    assert r.words.dtype == torch.int32 and r.words.is_cuda and r.cells == cells
    np.testing.assert_array_equal(N(r.words), R.pack(want))
    assert r.count() == int(want.sum()) and (P == 0) == (want.sum() == 0)
    if P == 10 ** 6:
        in_box, _ = R.cell_of(pts, lo, hi, cells)
        assert 0.2 < in_box.mean() < 0.8                                         # points outside the box mark nothing
    # marking twice changes nothing; marking into non-zero words keeps them and adds only the points' cells
    again = ops.region_mark(t, r.box(), cells, r.words.clone())
    assert torch.equal(again, r.words)
    before = np.random.RandomState(1).rand(*cells) < 0.1
    words = torch.from_numpy(R.pack(before)).to(cuda)
    ops.region_mark(t, r.box(), cells, words)
    np.testing.assert_array_equal(N(words), R.pack(G.mark(pts, lo, hi, cells, before)))
    R.unpack(N(words), cells)                                                    # tail bits zero
    # with dilation: occupancy's dilate on the marked set
    np.testing.assert_array_equal(N(Region.from_points(t, lo, hi, cells, dilate=2).words), R.pack(R.dilate(want, 2)))


def test_from_points_default_box(cuda):
    rs = np.random.RandomState(4)
    pts = (rs.uniform(-1, 1, (5000, 3)) * [1.0, 0.3, 2.0] + [0, 5, -3]).astype(np.float32)
    pts[:2] = [[np.nan, 0, 0], [0, np.inf, 0]]
    r = Region.from_points(torch.from_numpy(pts).to(cuda), cells=(32, 16, 48), dilate=1)
    lo, hi = G.default_box(pts, (32, 16, 48), 1)
    np.testing.assert_array_equal(r.bmin, lo)
    np.testing.assert_array_equal(r.bmax, hi)
    want = R.dilate(G.mark(pts, lo, hi, (32, 16, 48)), 1)
    np.testing.assert_array_equal(N(r.words), R.pack(want))
    assert 0 < r.fraction() < 1


def test_lookup_equals_restatement(cuda):
    reg = random_cells(CELLS)
    r = make_region(reg, cuda)
    pts, lo, hi = seeded_points(200000, 3)
    got = r.contains(torch.from_numpy(pts).to(cuda))
    assert got.dtype == torch.bool and got.shape == (len(pts),)
    want = G.inside(pts, lo, hi, CELLS, reg)
    np.testing.assert_array_equal(N(got), want)
    assert not want[:3].any() and not want[4]                                    # NaN / inf / the upper corner: outside
    in_box, _ = R.cell_of(pts, lo, hi, CELLS)
    assert 0.1 < want.mean() < 0.5 and (~in_box).mean() > 0.2
    np.testing.assert_array_equal(want, ~R.keep(pts, lo, hi, CELLS, ~reg))       # the carved grid keeps the rest
    assert r.contains(torch.empty((0, 3), device=cuda)).shape == (0,)
    with pytest.raises(ValueError, match='the region on'):
        r.to('cpu').contains(torch.from_numpy(pts[:4]).to(cuda))


# ---- 2. accumulate ---------------------------------------------------------------------------------------------------------

def seeded_weights(B, S, seed, cuda):
    """Non-negative, sum over a ray <= 1 (what compositing produces)."""
    rs = np.random.RandomState(seed)
    w = rs.rand(B, S)
    w = (w / w.sum(1, keepdims=True) * rs.rand(B, 1) * 0.999).astype(np.float32)
    assert (w.astype(np.float64).sum(1) <= 1).all() and (w >= 0).all()
    return torch.from_numpy(w).to(cuda)


@pytest.mark.parametrize('B,S', [(1, 64), (777, 64), (5000, 128), (16, 2), (1031, 192)])
def test_accumulate_equals_restatement(B, S, cuda):
    """Against the fp64 sum of the fp32 inputs: |err| <= S * 2^-24 * sum_j w_j per ray, the bound for an fp32 summation of S
    non-negative terms in any order (each of at most S - 1 additions rounds a partial sum that is <= the total, relative
    error 2^-24).  Membership is exact: the points are formed in the kernels' expression and tested in fp32."""
    reg = random_cells(CELLS, seed=B)
    r = make_region(reg, cuda)
    rows = bench_rows(cuda, B, seed=S)
    z = ops.stratified_z(rows, S, True)
    w = seeded_weights(B, S, B + S, cuda)
    got = ops.region_accumulate(rows, z, w, r.box(), r.cells, r.words)
    assert got.shape == (B,) and got.dtype == torch.float32
    want, m = G.accumulate(points_np(rows, z), N(w), BOX[0], BOX[1], CELLS, reg)
    total = N(w).astype(np.float64).sum(1)
    err = np.abs(N(got).astype(np.float64) - want)
    print(f'B={B} S={S}: max err / bound {float((err / np.maximum(S * 2.0 ** -24 * total, 1e-300)).max()):.3f}, '
          f'inside fraction {m.mean():.3f}')
    assert (err <= S * 2.0 ** -24 * total).all()
    in_box, _ = R.cell_of(points_np(rows, z).reshape(-1, 3), BOX[0], BOX[1], CELLS)
    assert in_box.reshape(B, S).any(1).all() and (~in_box).reshape(B, S).any(1).all()       # the rays cross the box and leave it
    assert 0.1 < m.mean() < 0.6 and (want > 0).mean() > 0.4 and (want < total).all()
    # the lookup kernel on the same points: the same membership
    np.testing.assert_array_equal(N(r.contains(torch.from_numpy(points_np(rows, z)).to(cuda))).reshape(B, S), m)
    # reproducible bit for bit, and a ray's result does not depend on the call it is part of
    again = ops.region_accumulate(rows, z, w, r.box(), r.cells, r.words)
    assert torch.equal(got.view(torch.int32), again.view(torch.int32))
    for h in (B // 2, B // 2 + 1):
        parts = [ops.region_accumulate(rows[a:b].contiguous(), z[a:b].contiguous(), w[a:b].contiguous(), r.box(), r.cells, r.words)
                 for a, b in ((0, h), (h, B))]
        assert torch.equal(torch.cat(parts).view(torch.int32), got.view(torch.int32))
    # a NaN weight outside the region does not reach the sum (a select, not a product)
    b, j = np.argwhere(~m)[len(np.argwhere(~m)) // 2]
    w2 = w.clone()
    w2[b, j] = float('nan')
    got2 = ops.region_accumulate(rows, z, w2, r.box(), r.cells, r.words)
    assert torch.isfinite(got2).all() and torch.equal(got2.view(torch.int32), got.view(torch.int32))
    b, j = np.argwhere(m)[0]                                                     # inside, it does
    w2 = w.clone()
    w2[b, j] = float('nan')
    got2 = ops.region_accumulate(rows, z, w2, r.box(), r.cells, r.words)
    assert torch.isnan(got2[b]) and int(torch.isnan(got2).sum()) == 1


def test_accumulate_empty_and_shape_errors(cuda):
    r = make_region(random_cells(CELLS), cuda)
    rows = bench_rows(cuda, 8)
    z = ops.stratified_z(rows, 64, True)
    assert ops.region_accumulate(rows[:0].contiguous(), z[:0].contiguous(), z[:0].contiguous(), r.box(), r.cells, r.words).shape == (0,)
    from mvip_nerf_amd._lib import MvipError
    with pytest.raises(MvipError, match='region_accumulate'):
        ops.region_accumulate(rows, z, z[:, :32].contiguous(), r.box(), r.cells, r.words)
    with pytest.raises(MvipError, match='region_accumulate'):
        ops.region_accumulate(rows, z, z, r.box(), r.cells, r.words[:-1].contiguous())
    none = make_region(np.zeros(CELLS, bool), cuda)
    full = make_region(np.ones(CELLS, bool), cuda)
    w = seeded_weights(8, 64, 0, cuda)
    assert not ops.region_accumulate(rows, z, w, none.box(), none.cells, none.words).any()
    in_box, _ = R.cell_of(points_np(rows, z).reshape(-1, 3), BOX[0], BOX[1], CELLS)
    want = np.where(in_box.reshape(8, 64), N(w).astype(np.float64), 0).sum(1)     # the whole box is not the whole ray
    np.testing.assert_allclose(N(ops.region_accumulate(rows, z, w, full.box(), full.cells, full.words)), want, rtol=64 * 2.0 ** -24)


# ---- 3. render_rays(..., region=) -------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def mlp(cuda):
    """The seeded 8x256 pair with a density head that renders something (the construction of tests/test_occupancy.py,
    written again): alpha_linear rescaled to sigma' = 4 (sigma - median) / std over the camera's sample points."""
    from oracle.weights import seeded_state_dict
    _, te, _, _, _ = run.create_nerf(bench.make_args(), device=cuda)
    rows = bench_rows(cuda, 2000, seed=99)
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


def render(te, rows, **kw):
    return run.render_rays(rows, te['network_fn'], te['network_query_fn'], 64, lindisp=True, N_importance=64,
                           network_fine=te['network_fine'], white_bkgd=True, **kw)


def assert_same(a, b, what=''):
    assert sorted(a) == sorted(b), (sorted(a), sorted(b))
    for k in a:
        x, y = N(a[k]), N(b[k])
        assert x.shape == y.shape and x.dtype == y.dtype, (what, k)
        np.testing.assert_array_equal(x, y, err_msg=f'{what} {k}')              # bit-equal (NaN == NaN)


@pytest.mark.parametrize('route,B', [('fused', 777), ('chain', 5000), ('occupancy', 777)])
def test_region_map_is_the_accumulate_pass_on_the_calls_own_outputs(route, B, mlp, cuda, monkeypatch):
    calls = {'fused': 0, 'compact': 0}
    fine_fused, compact = ops.render_fine_fused, ops.occupancy_compact
    monkeypatch.setattr(ops, 'render_fine_fused', lambda *a, **k: (calls.__setitem__('fused', calls['fused'] + 1), fine_fused(*a, **k))[1])
    monkeypatch.setattr(ops, 'occupancy_compact', lambda *a, **k: (calls.__setitem__('compact', calls['compact'] + 1), compact(*a, **k))[1])
    reg = random_cells(CELLS, seed=B)
    r = make_region(reg, cuda)
    rows = bench_rows(cuda, B, seed=B)
    kw = {}
    if route == 'occupancy':
        kw['occupancy'] = OccupancyGrid(BOX[0], BOX[1], CELLS, torch.from_numpy(R.pack(np.ones(CELLS, bool))).to(cuda))
    with torch.no_grad():
        ref = render(mlp, rows, retraw=True, need_alpha=True, **kw)
        assert 'region_map' not in ref                                           # region=None adds no key
        got = render(mlp, rows, retraw=True, need_alpha=True, region=r, **kw)
    assert calls == {'fused': 2 * (route == 'fused'), 'compact': 4 * (route == 'occupancy')}, calls
    m = got.pop('region_map')
    assert_same(got, ref, route)                                                 # every other key: the call without `region`
    assert m.shape == (B,) and m.dtype == torch.float32 and not m.requires_grad
    own = ops.region_accumulate(rows, got['z_vals'], got['weights'], r.box(), r.cells, r.words)
    assert torch.equal(m.view(torch.int32), own.view(torch.int32))
    want, inside = G.accumulate(points_np(rows, got['z_vals']), N(got['weights']), BOX[0], BOX[1], CELLS, reg)
    total = N(got['weights']).astype(np.float64).sum(1)
    assert (np.abs(N(m) - want) <= 128 * 2.0 ** -24 * total).all()
    assert want.max() > 0.1 and (want < total).any() and 0.1 < inside.mean() < 0.9


def test_region_map_with_autograd_on_and_through_render(mlp, cuda):
    r = make_region(random_cells(CELLS, seed=3), cuda)
    rows = bench_rows(cuda, 300, seed=5)
    out = render(mlp, rows, region=r)                                            # autograd on: the training chain
    assert out['rgb_map'].requires_grad and not out['region_map'].requires_grad and out['region_map'].grad_fn is None
    with torch.no_grad():
        ref = render(mlp, rows, region=r)
    assert torch.equal(out['region_map'], ref['region_map'])
    # render / batchify_rays pass the keyword through and reshape the map to the frame; chunks do not change it
    H, W = 30, 40
    focal, pose = bench.FOCAL * W / bench.W, bench.orbit_pose(0, cuda)
    kw = dict(mlp, near=bench.NEAR, far=bench.FAR, region=r)
    with torch.no_grad():
        a = run.render(H, W, focal, chunk=500, c2w=pose, **kw)[4]['region_map']
        b = run.render(H, W, focal, chunk=H * W, c2w=pose, **kw)[4]['region_map']
        soft, hard = propagate_masks(mlp, (H, W, focal), torch.stack([pose[:3, :4], bench.orbit_pose(2, cuda)[:3, :4]]), r,
                                     bench.NEAR, bench.FAR, threshold=0.25, chunk=700)
    assert a.shape == (H, W) and torch.equal(a, b)
    assert soft.shape == (2, H, W) and soft.dtype == torch.float32 and hard.dtype == torch.bool
    assert torch.equal(soft[0], a) and torch.equal(hard, soft >= 0.25) and not torch.equal(soft[0], soft[1])


def test_render_refusals_on_device(mlp, cuda):
    r = make_region(random_cells(CELLS), cuda)
    rows = bench_rows(cuda, 64)
    with torch.no_grad():
        with pytest.raises(ValueError, match='region.Region'):
            render(mlp, rows, region=r.carve())
        with pytest.raises(ValueError, match='region is on'):
            render(mlp, rows, region=r.to('cpu'))
        with pytest.raises(ValueError, match='11 columns'):
            render(mlp, rows[:, :8].contiguous(), region=r)
        render(mlp, rows, region=r)                                              # and the accepted call


# ---- 4. carve ----------------------------------------------------------------------------------------------------------------

def masked_chain(te, rows, keep_cells, box=BOX):
    """render_rays' six-launch chain (64 + 64 samples, lindisp, white background, no perturbation) with the network's raw
    output zeroed where the restatement says the grid `keep_cells` does not keep the sample: the definition of a render with
    an occupancy grid (the construction of tests/test_occupancy.py, written again)."""
    dev, B = rows.device, rows.shape[0]

    def masked(z, net):
        m = R.keep(points_np(rows, z).reshape(-1, 3), box[0], box[1], keep_cells.shape, keep_cells).reshape(z.shape)
        raw = net.query_rays(rows, z)
        return torch.where(torch.from_numpy(m).to(dev)[..., None], raw, torch.zeros_like(raw)), float(m.mean())

    z = ops.stratified_z(rows, 64, True, None)
    raw, k0 = masked(z, te['network_fn'])
    rgb, disp, acc, w, depth, alpha = ops.composite(raw, z, rows, None, True, False, True)
    ret = dict(rgb0=rgb, disp0=disp, acc0=acc, alpha0=alpha)
    _, z, z_std, _, _ = ops.sample_pdf_merge(z, w, _uniforms((B,), 64, True, False, dev))
    raw, k1 = masked(z, te['network_fine'])
    rgb, disp, acc, w, depth, alpha = ops.composite(raw, z, rows, None, True, False, True)
    ret.update(rgb_map=rgb, disp_map=disp, acc_map=acc, depth_map=depth, weights=w, z_vals=z, raw=raw, alpha=alpha, z_std=z_std)
    return ret, k0, k1


def test_carved_render_equals_masked_chain(mlp, cuda):
    """render_kwargs['occupancy'] = region.carve(): every key equals the chain with the raw output zeroed at the samples
    INSIDE the region, bit for bit; and nothing of the ray's weight is left inside the region."""
    reg = random_cells(CELLS, seed=21)
    r = make_region(reg, cuda)
    grid = r.carve()
    np.testing.assert_array_equal(N(grid.words), R.pack(~reg))
    rows = bench_rows(cuda, 3000, seed=11)
    with torch.no_grad():
        got = render(mlp, rows, retraw=True, need_alpha=True, occupancy=grid, region=r)
        ref, k0, k1 = masked_chain(mlp, rows, ~reg)
        plain = render(mlp, rows)
    assert 0.2 < k0 < 0.95 and 0.2 < k1 < 0.95
    m = got.pop('region_map')
    assert_same(got, ref, 'carve')
    assert not m.any()                                                           # the region is cut out
    assert not torch.equal(plain['rgb_map'], got['rgb_map'])


# ---- 5. end to end on an analytic scene ------------------------------------------------------------------------------------

C_A, R_A = np.array([0.0, 0.0, 0.0]), 0.5
C_B, R_B = np.array([0.9, 0.0, 1.5]), 0.25
WALL_Z = -1.5
A_H, A_W, A_FOCAL, A_NEAR, A_FAR = 128, 192, 200.0, 2.0, 7.0
A_VIEWS = [(0.0, 0.0), (-0.6, 0.0), (0.6, 0.2), (1.4, 0.0)]
A_BAND_SHARE = [0.31, 0.31, 0.31, 0.65]


def analytic_field(pts):
    """raw [B, S, 4]: sigma = 1e4 inside ball A, ball B or behind the wall z < -1.5, else 0; colour 0."""
    p = pts.double()
    ca, cb = (torch.tensor(c, device=p.device, dtype=torch.float64) for c in (C_A, C_B))
    solid = ((p - ca).norm(dim=-1) < R_A) | ((p - cb).norm(dim=-1) < R_B) | (p[..., 2] < WALL_Z)
    raw = torch.zeros(tuple(pts.shape[:-1]) + (4,), device=pts.device, dtype=torch.float32)
    raw[..., 3] = torch.where(solid, 1e4, 0.0).float()
    return raw


def analytic_pose(tx, ty, device):
    c = torch.eye(4, device=device)[:3].clone()
    c[:, 3] = torch.tensor([tx, ty, 4.0], device=device)
    return c


def analytic_geometry(tx, ty):
    """Per pixel (raster order), in fp64: closest distance of the ray to A's and B's centres, and whether B hides A there (the
    ray passes within r_B of B's centre and B's centre is the nearer one along it).  get_rays' convention: direction
    ((i - W/2) / f, -(j - H/2) / f, -1), identity rotation."""
    j, i = np.meshgrid(np.arange(A_H, dtype=np.float64), np.arange(A_W, dtype=np.float64), indexing='ij')
    d = np.stack([(i - A_W * 0.5) / A_FOCAL, -(j - A_H * 0.5) / A_FOCAL, -np.ones_like(i)], -1).reshape(-1, 3)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    o = np.array([tx, ty, 4.0])
    ta, tb = ((C_A - o) * d).sum(1), ((C_B - o) * d).sum(1)
    da = np.linalg.norm(o + d * ta[:, None] - C_A, axis=1)
    db = np.linalg.norm(o + d * tb[:, None] - C_B, axis=1)
    return da, db, (db < R_B) & (tb < ta)


def test_masks_lifted_from_one_view_of_an_analytic_scene(cuda):
    """Annotate view (0, 0) with the analytic mask "first hit is A", lift, propagate to four views.  With c = 1/32 the cell
    edge, theta_v the angle at A's centre between camera v and camera 0 and m_v = c + r_A (1 - cos theta_v) (one cell of
    localisation plus the limb view 0 cannot see): every pixel whose hard mask differs from the analytic one lies in
    |d_A - r_A| <= m_v, or in |d_B - r_B| <= c with d_A < r_A + m_v.  Where B hides A (fourth view) no hidden A pixel outside
    B's band is masked.  The excluded bands are pure geometry and bounded, so they cannot hide a failure."""
    kw = dict(network_fn=analytic_field, network_fine=None, network_query_fn=lambda p, d, n: n(p), N_samples=64,
              N_importance=64, perturb=0., white_bkgd=False, raw_noise_std=0., lindisp=False, use_viewdirs=True, ndc=False)
    hwf = (A_H, A_W, A_FOCAL)
    poses = torch.stack([analytic_pose(tx, ty, cuda) for tx, ty in A_VIEWS])
    da0, _, hid0 = analytic_geometry(*A_VIEWS[0])
    mask0 = ((da0 < R_A) & ~hid0).reshape(A_H, A_W)
    assert 1500 < mask0.sum() < 0.2 * mask0.size
    region = Region.from_masks(kw, hwf, poses[:1], torch.from_numpy(mask0[None]).to(cuda), A_NEAR, A_FAR,
                               bmin=(-1, -1, -1), bmax=(1, 1, 1), cells=64, dilate=1)
    assert region.cells == (64, 64, 64) and 0 < region.fraction() < 0.05
    soft, hard = propagate_masks(kw, hwf, poses, region, A_NEAR, A_FAR)
    assert soft.shape == (4, A_H, A_W) and float(soft.min()) >= 0 and float(soft.max()) <= 1 + 1e-5
    c = 2.0 / 64
    cam0 = np.array([A_VIEWS[0][0], A_VIEWS[0][1], 4.0])
    for v, (tx, ty) in enumerate(A_VIEWS):
        da, db, hidden = analytic_geometry(tx, ty)
        gt = (da < R_A) & ~hidden
        got = N(hard[v]).reshape(-1)
        cam = np.array([tx, ty, 4.0])
        cos = float(((C_A - cam) * (C_A - cam0)).sum() / np.linalg.norm(C_A - cam) / np.linalg.norm(C_A - cam0))
        m_v = c + R_A * (1 - min(cos, 1.0))
        band_a = np.abs(da - R_A) <= m_v
        band_b = (np.abs(db - R_B) <= c) & (da < R_A + m_v)
        band = band_a | band_b
        wrong = got != gt
        iou = (got & gt).sum() / max((got | gt).sum(), 1)
        worst = float(np.abs(da[wrong & ~band_b] - R_A).max()) if (wrong & ~band_b).any() else 0.0
        print(f'view {(tx, ty)}: m_v {m_v:.4f}, IoU {iou:.4f}, {int(wrong.sum())} wrong pixels, {int((wrong & ~band).sum())} outside '
              f'the bands, worst |d_A - r_A| of a wrong pixel {worst:.4f}, band share of the object {band.sum() / gt.sum():.3f}, '
              f'of the frame {band.mean():.4f}')
        assert gt.sum() > 1500
        assert band.sum() / gt.sum() <= A_BAND_SHARE[v] and band.mean() <= 0.045
        assert not (wrong & ~band).any()
        if v == 3:
            hidden_a = (da < R_A) & hidden
            in_b_band = np.abs(db - R_B) <= c
            print(f'   hidden A pixels {int(hidden_a.sum())}, of which masked {int((got & hidden_a).sum())}')
            assert hidden_a.sum() > 100
            assert not (got & hidden_a & ~in_b_band).any()                       # occlusion awareness
        else:
            assert not ((da < R_A) & hidden).any()
    with pytest.raises(ValueError, match='nothing to lift'):
        Region.from_masks(kw, hwf, poses[:1], torch.zeros((1, A_H, A_W), dtype=torch.bool, device=cuda), A_NEAR, A_FAR)


# ---- 6. a trained field -----------------------------------------------------------------------------------------------------

def iou(a, b):
    return float((a & b).sum()) / max(float((a | b).sum()), 1.0)


def copy_baseline(masks, poses, annotated):
    """Mean IoU, over the views that are not annotated, of the nearest annotated view's mask copied unchanged (nearest by
    camera position): what masks give without geometry."""
    out = []
    for v in range(len(masks)):
        if v not in annotated:
            a = min(annotated, key=lambda k: np.linalg.norm(poses[k, :, 3] - poses[v, :, 3]))
            out.append(iou(masks[v], masks[a]))
    return float(np.mean(out))


@pytest.mark.slow
def test_trained_field_masks_from_one_view_beat_the_copy_baseline(cuda):
    """1,500 iterations on the scene-1 fixture (tools/render_occupancy_ab.py::train_scene1), the fixture's own mask of view 0
    lifted with the defaults (box from the marked points, 64 cells, one dilation round) and propagated to the 29 other views:
    the mean IoU against the fixture's masks is greater than that of copying view 0's mask unchanged (0.222).  The fixture's
    images are the inpainted rasters, so the region lands on the surfaces BEHIND the object's place and the dataset's
    silhouettes are an approximate target: no further margin is fixed.  The set [0, 15, 29] is computed and printed, not
    gated.  Measured (this test and tools/propagate_masks.py, one training run each): 0.796 / 0.797 for [0]; 0.700 / 0.699
    against a copy baseline of 0.585 for [0, 15, 29]."""
    from tools import render_occupancy_ab as T
    scene = T.train_scene1(cuda)
    d = np.load(T.FIXTURE)
    masks = d['masks'].astype(bool)
    poses_np = d['poses'][:, :, :4]
    hwf = (scene['H'], scene['W'], scene['focal'])
    assert masks.shape == (len(poses_np), scene['H'], scene['W'])
    for annotated in ([0], [0, 15, 29]):
        region = Region.from_masks(scene['te'], hwf, scene['poses'][annotated], torch.from_numpy(masks[annotated]).to(cuda),
                                   scene['near'], scene['far'])
        others = [v for v in range(len(masks)) if v not in annotated]
        _, hard = propagate_masks(scene['te'], hwf, scene['poses'][others], region, scene['near'], scene['far'])
        ious = [iou(N(hard[k]), masks[v]) for k, v in enumerate(others)]
        base = copy_baseline(masks, poses_np, annotated)
        print(f'annotated {annotated}: region {region.count()} of {region.n_cells} cells ({region.fraction():.4f}), mean IoU '
              f'{np.mean(ious):.4f} (min {np.min(ious):.4f}), copy baseline {base:.4f}')
        assert 0 < region.count() < region.n_cells
        if annotated == [0]:
            assert base == pytest.approx(0.222, abs=0.001)
            assert np.mean(ious) > base
