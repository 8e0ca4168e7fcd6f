"""Occupancy-grid empty-space skipping on the GPU (mvip_nerf_amd/occupancy.py, csrc/occupancy.hip, run.render_rays'
`occupancy` keyword): the build / dilate / lookup / compaction kernels against the numpy restatement
(tests/occupancy_numpy.py), and the renders against the DEFINITION -- the render the ordinary chain produces when the
network's raw output is replaced by zeros at every sample whose point lies in a cell the grid marks empty -- written here
from existing ops.  Grids of the render tests are model-independent (a ball, a seeded random cell field): a random-weight
field is too fine-grained to carve, a grid derived from it would pass with nothing skipped."""
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import occupancy_numpy as R                              # noqa: E402

import bench                                             # noqa: E402
from mvip_nerf_amd import mesh, ops, run                 # noqa: E402
from mvip_nerf_amd.occupancy import OccupancyGrid        # noqa: E402
from mvip_nerf_amd.run_nerf_helpers import NeRF, _uniforms   # noqa: E402

pytestmark = pytest.mark.gpu

# the camera of bench.orbit_pose(0) sits at (0, 0, 0.3) and looks down -z; its samples lie at depth 1.2 .. 7.74.  The box
# covers depths 1.0 .. 4.6: every ray enters it, every ray leaves it through the back, the outer ones through the sides.
BOX = ((-1.5, -1.2, -4.3), (1.5, 1.2, -0.7))
CELLS = (40, 33, 64)
# the boxes of the definition test, chosen on the CPU from the geometry alone so that the coarse pass keeps about half of
# its samples (0.51 / 0.54; a kept sample is outside the box or in an occupied cell).  The fine pass re-evaluates the 64
# coarse depths and adds 64 of its own, so its kept fraction lies between half the coarse one and (coarse + 1) / 2: inside
# 0.2 .. 0.8 whatever the network says.  'ball': the frustum runs along an edge of the box, through the ball's flank;
# 'random': the box holds 90 % of the samples.  Every ray enters its box and leaves it.
DEFINITION_BOXES = {'ball': ((-1.0, -0.8, -6.5), (3.0, 2.4, -0.5)), 'random': ((-2.5, -1.9, -6.5), (2.5, 1.9, -0.6))}


def N(t):
    return t.detach().cpu().numpy()


def ball_cells(cells, radius=0.45):
    ax = [(np.arange(c, dtype=np.float64) + 0.5) / c - 0.5 for c in cells]
    X, Y, Z = np.meshgrid(*ax, indexing='ij')
    return X * X + Y * Y + Z * Z <= radius * radius


def random_cells(cells, seed=7):
    return np.random.RandomState(seed).rand(*cells) < 0.5


def make_grid(occ, cuda, box=BOX):
    return OccupancyGrid(box[0], box[1], occ.shape, torch.from_numpy(R.pack(occ)).to(cuda))


def bench_rows(cuda, B, seed=0):
    sel = torch.from_numpy(np.random.RandomState(seed).randint(0, bench.H * bench.W, B)).to(cuda)
    return ops.ray_rows_from_pose(bench.orbit_pose(0, cuda), bench.H, bench.W, bench.FOCAL, bench.NEAR, bench.FAR, sel=sel)


@pytest.fixture(scope='module')
def mlp(cuda):
    """The seeded 8x256 pair with a density head that renders something: the seeded field's sigma is negative wherever the
    bench camera looks (every weight 0, every pixel the background), which would make the comparisons below vacuous, so
    alpha_linear is rescaled to sigma' = 4 (sigma - median) / std over the camera's sample points: half of them dense."""
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
    with torch.no_grad():
        acc = run.render_rays(rows, te['network_fn'], te['network_query_fn'], 64, lindisp=True, N_importance=64,
                              network_fine=te['network_fine'], white_bkgd=True)['acc_map']
    assert 0.2 < float(acc.mean()) and float(acc.std()) > 0.01
    return te


@pytest.fixture
def chain(monkeypatch):
    """occupancy=None renders take the six-launch chain (the two-launch fused form is bit-identical to it, tests/test_render.py)."""
    monkeypatch.setattr(run, 'FUSED_RENDER', False)


def set_precision(te, precision, fold=True):
    for net in (te['network_fn'], te['network_fine']):
        if isinstance(net, NeRF):
            net.inference_precision = precision
            net.fold_feature_inference = fold


def assert_same(a, b, what=''):
    assert sorted(a) == sorted(b), (sorted(a), sorted(b))
    for k in a:
        x, y = N(a[k]), N(b[k])
        assert x.shape == y.shape and x.dtype == y.dtype, (what, k)
        np.testing.assert_array_equal(x, y, err_msg=f'{what} {k}')            # bit-equal (NaN == NaN)


# ---- 1. build / dilate ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('cells,k', [((5, 3, 7), 1), ((40, 33, 64), 1), ((13, 9, 21), 2), ((6, 11, 5), 3), ((64, 1, 1), 2),
                                     ((1, 1, 1), 8)])
def test_build_and_dilate_equal_restatement_on_seeded_fields(cells, k, cuda):
    rs = np.random.RandomState(cells[0] * 100 + k)
    shape = tuple(c * k + 1 for c in cells)
    sigma = rs.randn(*shape).astype(np.float32)
    thr = float(np.quantile(sigma, 0.97 if k == 1 else 0.995))
    sigma.reshape(-1)[rs.randint(0, sigma.size, 3)] = np.nan                     # NaN counts as occupied
    sigma.reshape(-1)[rs.randint(0, sigma.size, 3)] = thr                        # sigma == threshold is empty
    s = torch.from_numpy(sigma).to(cuda)
    occ = R.build(sigma, thr, k)
    for rounds in (0, 1, 2):
        g = OccupancyGrid.from_density(s, (0, 0, 0), (1, 2, 3), thr, samples_per_cell=k, dilate=rounds)
        assert g.cells == cells and g.words.dtype == torch.int32 and g.words.is_cuda
        np.testing.assert_array_equal(N(g.words), R.pack(R.dilate(occ, rounds)), err_msg=f'dilate={rounds}')
        assert g.occupied_fraction() == pytest.approx(R.dilate(occ, rounds).mean())
    if min(cells) > 1:
        assert 0 < occ.mean() < 1 and R.dilate(occ, 1).mean() > occ.mean()
    g2 = OccupancyGrid.from_density(s, (0, 0, 0), (1, 2, 3), thr, samples_per_cell=k, dilate=2)
    assert torch.equal(g.words, g2.words)                                        # reproducible bit for bit


def test_build_on_a_network_field_is_neither_trivial_case(cuda):
    """oracle.mlp_init(0)'s sigma on [-1, 1]^3 at 65 points per axis, threshold at the field's 0.95 quantile: about a
    fifth of the 64^3 cells occupied undilated and about half with one dilation round (21.7 % / 55.9 % on the CPU oracle)."""
    from oracle import nerf_oracle as O
    _, te, _, _, _ = run.create_nerf(bench.make_args(), device=cuda)
    te['network_fine'].load_state_dict(O.mlp_init(0))
    lo, hi = (-1, -1, -1), (1, 1, 1)
    sigma = mesh.density_grid(te, lo, hi, 65, network='fine')
    thr = float(np.quantile(N(sigma).astype(np.float64), 0.95))
    assert thr > 0
    occ = R.build(N(sigma), thr, 1)
    g0 = OccupancyGrid.from_density(sigma, lo, hi, thr, dilate=0)
    g1 = OccupancyGrid.from_density(sigma, lo, hi, thr, dilate=1)
    np.testing.assert_array_equal(N(g0.words), R.pack(occ))
    np.testing.assert_array_equal(N(g1.words), R.pack(R.dilate(occ)))
    print(f'occupied: {g0.occupied_fraction():.4f} undilated, {g1.occupied_fraction():.4f} dilated')
    assert 0.15 < g0.occupied_fraction() < 0.30 and 0.45 < g1.occupied_fraction() < 0.65
    # from_model on one network = density_grid + from_density
    gm = OccupancyGrid.from_model(te, lo, hi, cells=64, threshold=thr, samples_per_cell=1, dilate=1, networks=('fine',))
    assert torch.equal(gm.words, g1.words)
    both = OccupancyGrid.from_model(te, lo, hi, cells=64, threshold=thr, samples_per_cell=1, dilate=1)
    coarse = OccupancyGrid.from_model(te, lo, hi, cells=64, threshold=thr, samples_per_cell=1, dilate=1, networks=('coarse',))
    assert torch.equal(both.words, g1.words | coarse.words)


# ---- 2. lookup and the mark / compact pass ----------------------------------------------------------------------------------

def test_lookup_equals_restatement(cuda):
    occ = random_cells(CELLS)
    g = make_grid(occ, cuda)
    rs = np.random.RandomState(3)
    lo, hi = np.float32(BOX[0]), np.float32(BOX[1])
    pts = (lo + (hi - lo) * rs.uniform(-0.2, 1.2, (200000, 3))).astype(np.float32)
    pts[:6] = [[np.nan, 0, -2], [0, np.inf, -2], [0, 0, -np.inf], lo, hi, (lo + hi) / 2]
    faces = lo + (hi - lo) * (rs.randint(0, 41, (1000, 3)) / np.float32(40))      # cell faces along x, box faces included
    pts[100:1100] = faces.astype(np.float32)
    got = g.lookup(torch.from_numpy(pts).to(cuda))
    assert got.dtype == torch.bool and got.shape == (len(pts),)
    want = R.keep(pts, lo, hi, CELLS, occ)
    np.testing.assert_array_equal(N(got), want)
    assert want[:3].all() and want[4]                                            # NaN / inf / the upper corner: outside, kept
    assert 0.3 < want.mean() < 0.9


# (66000, 128): 8250 workgroups, the smallest round size past one 8192-count chunk of the scan of the workgroup counts
@pytest.mark.parametrize('B,S', [(1, 64), (777, 64), (5000, 128), (16, 2), (1031, 7), (66000, 128)])
def test_mark_and_compact_equal_restatement(B, S, cuda):
    occ = random_cells(CELLS, seed=B)
    g = make_grid(occ, cuda)
    rows = bench_rows(cuda, B, seed=S)
    if B > 10:
        rows[5, 0] = float('nan')                                                # a NaN origin: every sample of the ray is kept
    z = ops.stratified_z(rows, S, True)
    idx, pts, dirs, K, mask, full = ops.occupancy_compact(rows, z, g.box(), g.cells, g.words, want_mask=True, want_pts=True)
    assert idx.dtype == torch.int32 and mask.dtype == torch.uint8 and full.shape == (B, S, 3)
    want = R.keep(N(full).reshape(-1, 3), BOX[0], BOX[1], CELLS, occ)            # on the pass's own emitted points
    np.testing.assert_array_equal(N(mask).reshape(-1).astype(bool), want)
    np.testing.assert_array_equal(N(idx), np.nonzero(want)[0])                   # ascending
    assert K == int(want.sum()) == idx.shape[0]
    if B * S > 8192 * 1024:
        assert N(idx)[-1] >= 8192 * 1024                                         # the carry into the second chunk decides an output
    np.testing.assert_array_equal(N(pts), N(full).reshape(-1, 3)[N(idx)])
    np.testing.assert_array_equal(N(dirs), N(rows)[N(idx) // S, 8:11])
    ref = N(rows[:, None, 0:3] + rows[:, None, 3:6] * z[:, :, None])
    ulp = np.spacing(np.abs(ref).astype(np.float32))
    with np.errstate(invalid='ignore'):
        assert np.all((np.abs(N(full) - ref) <= ulp) | np.isnan(ref))            # within 1 ulp of o + d z (expected: equal)
    inside, _ = R.cell_of(N(full).reshape(-1, 3), BOX[0], BOX[1], CELLS)
    if B > 10:
        assert (~inside).sum() > 0 and want[~inside].all()                       # rays leave the box: those samples are kept
        assert N(mask)[5].all()
    # the same call without the optional outputs, and again: identical
    idx2, pts2, dirs2, K2, m2, f2 = ops.occupancy_compact(rows, z, g.box(), g.cells, g.words)
    assert m2 is None and f2 is None and K2 == K
    assert torch.equal(idx, idx2) and torch.equal(pts.view(torch.int32), pts2.view(torch.int32)) and torch.equal(dirs.view(torch.int32), dirs2.view(torch.int32))
    # scatter: values at idx, zeros elsewhere
    raw_k = torch.randn(K, 4, device=cuda)
    raw = ops.scatter_raw(raw_k, idx, (B, S))
    want_raw = np.zeros((B * S, 4), np.float32)
    want_raw[N(idx)] = N(raw_k)
    np.testing.assert_array_equal(N(raw).reshape(-1, 4), want_raw)


def test_compact_empty_inputs(cuda):
    g = make_grid(random_cells(CELLS), cuda)
    rows = bench_rows(cuda, 4)[:0].contiguous()
    z = torch.empty((0, 64), device=cuda)
    idx, pts, dirs, K, _, _ = ops.occupancy_compact(rows, z, g.box(), g.cells, g.words)
    assert K == 0 and idx.shape == (0,) and pts.shape == (0, 3) and dirs.shape == (0, 3)
    assert ops.scatter_raw(torch.empty((0, 4), device=cuda), idx, (0, 64)).shape == (0, 64, 4)
    raw = ops.scatter_raw(torch.empty((0, 4), device=cuda), idx, (3, 5))
    assert raw.shape == (3, 5, 4) and not raw.any()


# ---- the masked chain: the definition, from existing ops ----------------------------------------------------------------

def masked_chain(te, rows, occ, S, Nf, lindisp, white, perturb=0., pytest_=False, box=BOX, z_fine=None):
    """render_rays' six-launch chain with the network's raw output zeroed where the restatement says "empty".  Returns
    (dict, kept fraction coarse, kept fraction fine).  z_fine: depths to use for the fine stage instead of the chain's own."""
    dev, B = rows.device, rows.shape[0]
    qfn = te['network_query_fn']
    coarse = te['network_fn']
    fine = te['network_fine'] if te['network_fine'] is not None else coarse

    def points(z):
        return rows[:, None, 0:3] + rows[:, None, 3:6] * z[:, :, None]

    def query(z, net):
        if isinstance(net, NeRF) and getattr(qfn, '_mvip_native', False):
            return net.query_rays(rows, z)
        return qfn(points(z), rows[:, 8:11], net)

    def masked(z, net):
        m = R.keep(N(points(z)).reshape(-1, 3), box[0], box[1], occ.shape, occ).reshape(z.shape)
        m = torch.from_numpy(m).to(dev)
        raw = query(z, net)
        return torch.where(m[..., None], raw, torch.zeros_like(raw)), float(m.float().mean())

    t_rand = None
    if perturb > 0.:
        t_rand = torch.rand((B, S), device=dev)
        if pytest_:
            np.random.seed(0)
            t_rand = torch.tensor(np.random.rand(B, S), dtype=torch.float32, device=dev)
    z = ops.stratified_z(rows, S, lindisp, t_rand)
    raw, k0 = masked(z, coarse)
    rgb, disp, acc, w, depth, alpha = ops.composite(raw, z, rows, None, white, False, True)
    ret, k1 = {}, None
    if Nf > 0:
        ret.update(rgb0=rgb, disp0=disp, acc0=acc, alpha0=alpha)
        u = _uniforms((B,), Nf, perturb == 0., pytest_, dev)
        _, z, z_std, _, _ = ops.sample_pdf_merge(z, w, u)
        ret['z_std'] = z_std
        if z_fine is not None:
            z = z_fine
        raw, k1 = masked(z, fine)
        rgb, disp, acc, w, depth, alpha = ops.composite(raw, z, rows, None, white, False, True)
        ret['alpha'] = alpha
    ret.update(rgb_map=rgb, disp_map=disp, acc_map=acc, depth_map=depth, weights=w, z_vals=z, raw=raw)
    return ret, k0, k1


def grid_render(te, rows, grid, S, Nf, lindisp, white, perturb=0., pytest_=False):
    grid.reset_stats()
    out = run.render_rays(rows, te['network_fn'], te['network_query_fn'], S, retraw=True, lindisp=lindisp, perturb=perturb,
                          N_importance=Nf, network_fine=te['network_fine'], white_bkgd=white, pytest=pytest_,
                          need_alpha=Nf > 0, occupancy=grid)
    s = grid.stats
    return out, s['kept_coarse'] / max(1, s['samples_coarse']), (s['kept_fine'] / s['samples_fine'] if s['samples_fine'] else None)


# ---- 3. full grid == the ordinary render ----------------------------------------------------------------------------------

@pytest.mark.parametrize('precision', [0, 1], ids=['f32', 'f16x3'])
@pytest.mark.parametrize('white', [True, False], ids=['white', 'black'])
@pytest.mark.parametrize('mode', ['test', 'train'])
@pytest.mark.parametrize('B', [1, 777, 5000])
def test_full_grid_equals_ordinary_render_bitwise(B, mode, white, precision, mlp, chain, cuda):
    """All bits set: every sample is kept, so every key equals the six-launch chain's.  Expected and asserted BIT-EQUAL:
    the points and rays entry points instantiate one kernel template, per-point arithmetic does not depend on the
    neighbours in the tile, and the compaction forms the point with the ray kernels' expression (no fma contraction: the
    library is built with -ffp-contract=off)."""
    set_precision(mlp, precision)
    try:
        grid = make_grid(np.ones(CELLS, bool), cuda)
        rows = bench_rows(cuda, B, seed=B)
        perturb, pyt = (1., True) if mode == 'train' else (0., False)
        with torch.no_grad():
            got, k0, k1 = grid_render(mlp, rows, grid, 64, 64, True, white, perturb, pyt)
            ref = run.render_rays(rows, mlp['network_fn'], mlp['network_query_fn'], 64, retraw=True, lindisp=True,
                                  perturb=perturb, N_importance=64, network_fine=mlp['network_fine'], white_bkgd=white,
                                  pytest=pyt, need_alpha=True)
        assert k0 == 1.0 and k1 == 1.0 and grid.stats['network_launches'] == 2
        assert_same(got, ref, f'B={B} {mode}')
    finally:
        set_precision(mlp, 0)


# ---- 4. empty grid: nothing evaluated -----------------------------------------------------------------------------------------

@pytest.mark.parametrize('white', [True, False], ids=['white', 'black'])
def test_empty_grid_launches_no_network_kernel(white, mlp, cuda, monkeypatch):
    def boom(*a, **k):
        raise AssertionError('a network kernel was launched')
    for name in ('mlp_points', 'mlp_rays', 'render_coarse_fused', 'render_fine_fused'):
        monkeypatch.setattr(ops, name, boom)
    grid = make_grid(np.zeros((8, 8, 8), bool), cuda, box=((-20, -20, -20), (20, 20, 20)))      # contains every sample
    rows = bench_rows(cuda, 300)
    with torch.no_grad():
        out, k0, k1 = grid_render(mlp, rows, grid, 64, 64, True, white)
    assert k0 == 0.0 and k1 == 0.0 and grid.stats['network_launches'] == 0
    assert grid.stats['samples_coarse'] == 300 * 64 and grid.stats['samples_fine'] == 300 * 128
    assert not out['acc_map'].any() and not out['weights'].any() and not out['acc0'].any() and not out['raw'].any()
    for k in ('rgb_map', 'rgb0'):
        assert torch.equal(out[k], torch.full_like(out[k], 1.0 if white else 0.0))
    assert out['weights'].shape == (300, 128) and out['z_vals'].shape == (300, 128)


# ---- 5. the definition ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('precision,fold', [(0, True), (0, False), (1, True)], ids=['f32-fold', 'f32-nofold', 'f16x3'])
@pytest.mark.parametrize('kind', ['ball', 'random'])
def test_grid_render_equals_masked_chain(kind, precision, fold, mlp, cuda):
    """Every key of the grid render equals the masked chain (stratified_z -> query_rays -> where(mask, raw, 0) -> composite
    -> sample_pdf_merge -> the same again), bit for bit, on a ball of radius 0.45 of the box and on a seeded 50 % cell
    field; both passes keep between 20 % and 80 % of their samples, so neither the skipping nor the keeping is trivial."""
    set_precision(mlp, precision, fold)
    try:
        occ = ball_cells(CELLS) if kind == 'ball' else random_cells(CELLS)
        box = DEFINITION_BOXES[kind]
        grid = make_grid(occ, cuda, box)
        rows = bench_rows(cuda, 3000, seed=11)
        with torch.no_grad():
            got, k0, k1 = grid_render(mlp, rows, grid, 64, 64, True, True)
            ref, r0, r1 = masked_chain(mlp, rows, occ, 64, 64, True, True, box=box)
        inside, _ = R.cell_of(N(rows[:, None, 0:3] + rows[:, None, 3:6] * got['z_vals'][:, :, None]).reshape(-1, 3), box[0], box[1], CELLS)
        inside = inside.reshape(3000, -1)
        assert inside.any(1).all() and (~inside).any(1).all()                    # every ray crosses the box and leaves it
        print(f'{kind}: kept {k0:.3f} of the coarse samples, {k1:.3f} of the fine samples')
        assert 0.2 < k0 < 0.8 and 0.2 < k1 < 0.8
        assert k0 == pytest.approx(r0, abs=1e-6) and k1 == pytest.approx(r1, abs=1e-6)
        assert grid.stats['network_launches'] == 2
        assert_same(got, ref, kind)
        # skipping changed the picture: the definition is not the ordinary render on these grids
        with torch.no_grad():
            plain = run.render_rays(rows, mlp['network_fn'], mlp['network_query_fn'], 64, lindisp=True, N_importance=64,
                                    network_fine=mlp['network_fine'], white_bkgd=True)
        assert not torch.equal(plain['rgb_map'], got['rgb_map'])
    finally:
        set_precision(mlp, 0)


def test_grid_render_train_mode_equals_masked_chain(mlp, cuda):
    occ = random_cells(CELLS, seed=5)
    grid = make_grid(occ, cuda)
    rows = bench_rows(cuda, 1200, seed=2)
    with torch.no_grad():
        got, k0, k1 = grid_render(mlp, rows, grid, 64, 64, True, False, 1., True)
        ref, _, _ = masked_chain(mlp, rows, occ, 64, 64, True, False, 1., True)
    assert 0 < k0 < 1 and 0 < k1 < 1
    assert_same(got, ref)


# ---- 6. chunks, render_path, N_importance = 0, the hash-grid model ----------------------------------------------------------

def small_frame(cuda):
    H, W = 60, 80
    return H, W, bench.FOCAL * W / bench.W, bench.orbit_pose(0, cuda)


def test_chunk_invariance_and_render_path_repeat_bitwise(mlp, cuda):
    H, W, focal, pose = small_frame(cuda)
    grid = make_grid(ball_cells(CELLS), cuda)
    kw = dict(mlp, near=bench.NEAR, far=bench.FAR, occupancy=grid)
    with torch.no_grad():
        a = run.render(H, W, focal, chunk=1000, c2w=pose, retraw=True, **kw)
        b = run.render(H, W, focal, chunk=H * W, c2w=pose, retraw=True, **kw)
        c = run.render(H, W, focal, chunk=1 << 15, c2w=pose, retraw=True, **dict(kw, occupancy=None))
    for x, y in zip(a[:4], b[:4]):
        assert torch.equal(x, y)
    assert_same(a[4], b[4])
    assert not torch.equal(a[0], c[0])
    poses = torch.stack([bench.orbit_pose(k, cuda) for k in (0, 3)], 0)
    grid.reset_stats()
    r1, d1, _ = run.render_path(poses, (H, W, focal), 2048, kw)
    kept = grid.stats['kept_fine'] / grid.stats['samples_fine']
    r2, d2, _ = run.render_path(poses, (H, W, focal), 2048, kw)
    assert r1.shape == (2, H, W, 3) and 0 < kept < 1
    np.testing.assert_array_equal(r1, r2)
    np.testing.assert_array_equal(d1, d2)
    np.testing.assert_array_equal(r1[0], N(a[0]))


def test_no_importance_sampling(mlp, cuda):
    occ = ball_cells(CELLS)
    grid = make_grid(occ, cuda)
    rows = bench_rows(cuda, 900, seed=4)
    te = dict(mlp, network_fine=None)
    with torch.no_grad():
        grid.reset_stats()
        got = run.render_rays(rows, te['network_fn'], te['network_query_fn'], 64, retraw=True, lindisp=True, N_importance=0,
                              network_fine=None, white_bkgd=True, occupancy=grid)
        ref, _, _ = masked_chain(te, rows, occ, 64, 0, True, True)
    assert grid.stats['samples_fine'] == 0 and 0 < grid.stats['kept_coarse'] < grid.stats['samples_coarse']
    assert sorted(got) == ['acc_map', 'depth_map', 'disp_map', 'raw', 'rgb_map', 'weights', 'z_vals']
    assert_same(got, {k: ref[k] for k in got})


def test_hash_grid_model_equals_its_masked_chain(cuda):
    args = types.SimpleNamespace(
        use_viewdirs=True, N_importance=64, alpha_model_path=None, netchunk=65536, lrate=1e-2, basedir='/tmp/x',
        expname='none', ft_path=None, no_reload=True, perturb=0., N_samples=64, white_bkgd=True, raw_noise_std=0.,
        dataset_type='llff', no_ndc=True, lindisp=True)
    torch.manual_seed(0)
    _, te, _, _, _ = run.create_nerf_tcnn(args, cuda)
    with torch.no_grad():                                 # tables with visible structure (the seeded ones are ~1e-4)
        for net, seed in ((te['network_fn'], 5), (te['network_fine'], 6)):
            g = torch.Generator().manual_seed(seed)
            net.encoder.params.copy_(torch.rand(net.encoder.params.shape, generator=g) * 2 - 1)
    occ = random_cells(CELLS, seed=9)
    grid = make_grid(occ, cuda)
    rows = bench_rows(cuda, 1500, seed=8)
    with torch.no_grad():
        got, k0, k1 = grid_render(te, rows, grid, 64, 64, True, True)
        ref, _, _ = masked_chain(te, rows, occ, 64, 64, True, True)
    assert 0 < k0 < 1 and 0 < k1 < 1 and grid.stats['network_launches'] == 2
    assert_same(got, ref)


# ---- 7. refusals -------------------------------------------------------------------------------------------------------------

def test_refusals_on_device(mlp, cuda):
    grid = make_grid(ball_cells(CELLS), cuda)
    rows = bench_rows(cuda, 64)
    args = (rows, mlp['network_fn'], mlp['network_query_fn'], 64)
    kw = dict(lindisp=True, N_importance=64, network_fine=mlp['network_fine'], white_bkgd=True)
    with pytest.raises(ValueError, match='backward'):
        run.render_rays(*args, occupancy=grid, **kw)                             # autograd on, parameters require grad
    with torch.no_grad():
        with pytest.raises(ValueError, match='raw_noise_std'):
            run.render_rays(*args, occupancy=grid, raw_noise_std=1.0, **kw)
        with pytest.raises(ValueError, match='sigma_loss'):
            run.render_rays(*args, occupancy=grid, sigma_loss=object(), **kw)
        with pytest.raises(ValueError, match='grid is on'):
            run.render_rays(*args, occupancy=grid.to('cpu'), **kw)
        with pytest.raises(ValueError, match='the grid on'):
            grid.to('cpu').lookup(rows[:, :3])
        run.render_rays(*args, occupancy=grid, **kw)                             # and the accepted call
    for p in list(mlp['network_fn'].parameters()) + list(mlp['network_fine'].parameters()):
        p.requires_grad_(False)
    try:
        run.render_rays(*args, occupancy=grid, **kw)                             # frozen parameters: no backward asked for
    finally:
        for p in list(mlp['network_fn'].parameters()) + list(mlp['network_fine'].parameters()):
            p.requires_grad_(True)


# ---- 8. a trained field ---------------------------------------------------------------------------------------------------------

@pytest.mark.slow
def test_trained_field_default_grid_skips_and_keeps_psnr(cuda, tmp_path):
    """1,500 iterations on the scene-1 fixture (the recipe of test_configs.py's held-out PSNR test, through
    tools/render_occupancy_ab.py::train_scene1), the grid from OccupancyGrid.from_model with its default settings over the
    cameras' frustum box: the fine pass skips samples, and the held-out view's PSNR against the ground truth moves by less
    than 0.05 dB against the ordinary render of the same weights -- this project's criterion for "the same render"."""
    from tools import render_occupancy_ab as T
    scene = T.train_scene1(cuda)
    bmin, bmax = T.scene_bounds(scene)
    grid = OccupancyGrid.from_model(scene['te'], bmin, bmax)
    p = str(tmp_path / 'grid.npz')
    grid.save(p)
    grid = OccupancyGrid.load(p, cuda)
    H, W, focal = scene['H'], scene['W'], scene['focal']
    plain = T.render_view(scene, H, W, focal)[0]
    grid.reset_stats()
    skipped = T.render_view(scene, H, W, focal, grid)[0]
    kept = T.kept_fractions(grid)
    gt = scene['images'][scene['held']]
    p_plain, p_grid = T.psnr(plain, gt), T.psnr(skipped, gt)
    print(f'occupied {grid.occupied_fraction():.4f}; kept coarse {kept["coarse"]:.4f} fine {kept["fine"]:.4f}; PSNR vs ground '
          f'truth {p_plain:.4f} ordinary, {p_grid:.4f} grid; PSNR between the two renders (dB, None = identical): '
          f'{T.psnr(skipped, plain)}')
    assert p_plain > 20.0
    assert kept['fine'] < 1.0 and kept['coarse'] < 1.0
    assert abs(p_grid - p_plain) < 0.05, (p_grid, p_plain)
