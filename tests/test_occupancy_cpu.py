"""Occupancy grids without a GPU: the numpy restatement (tests/occupancy_numpy.py) on hand-made cases, the host side of
mvip_nerf_amd/occupancy.py (word layout, save / load, every ValueError) and the render_rays refusals that need no device."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import occupancy_numpy as R                              # noqa: E402

from mvip_nerf_amd import occupancy, run                 # noqa: E402
from mvip_nerf_amd.occupancy import OccupancyGrid        # noqa: E402


# ---- the restatement -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('k', [1, 2])
def test_single_point_marks_the_cells_that_own_it(k):
    cells = (4, 3, 5)
    shape = tuple(c * k + 1 for c in cells)
    for point in [(0, 0, 0), (k, k, k), (2 * k, k, 3 * k), (4 * k, 3 * k, 5 * k), (k, 0, 5 * k)] + ([(1, 1, 1), (2, 3, 4)] if k == 2 else []):
        sigma = np.zeros(shape, np.float32)
        sigma[point] = 2.0
        occ = R.build(sigma, 1.0, k)
        want = np.zeros(cells, bool)
        owners = []
        for p, c in zip(point, cells):
            # point p belongs to cell p // k, and also to cell p // k - 1 when it sits on the shared face
            o = [i for i in {p // k, p // k - 1 if p % k == 0 else p // k} if 0 <= i < c]
            owners.append(o)
        for i in owners[0]:
            for j in owners[1]:
                for l in owners[2]:
                    want[i, j, l] = True
        np.testing.assert_array_equal(occ, want)
        assert 1 <= occ.sum() <= 8
    # an interior lattice corner is owned by 8 cells
    sigma = np.zeros(shape, np.float32)
    sigma[k, k, k] = 2.0
    assert R.build(sigma, 1.0, k).sum() == 8


def test_threshold_equality_is_empty_and_nan_is_occupied():
    sigma = np.full((3, 3, 3), 1.0, np.float32)
    assert not R.build(sigma, 1.0).any()                         # sigma == threshold: empty
    assert R.build(sigma, np.nextafter(np.float32(1.0), np.float32(0.0))).all()
    sigma[:] = 0
    sigma[2, 2, 2] = np.nan
    occ = R.build(sigma, 0.0)
    assert occ.sum() == 1 and occ[1, 1, 1]
    sigma[2, 2, 2] = -np.inf
    assert not R.build(sigma, 0.0).any()
    sigma[2, 2, 2] = np.inf
    assert R.build(sigma, 0.0).sum() == 1


def test_dilation_is_clipped_at_the_faces():
    occ = np.zeros((4, 5, 6), bool)
    occ[0, 0, 0] = True
    d = R.dilate(occ)
    assert d.sum() == 8 and d[:2, :2, :2].all()
    occ[:] = False
    occ[2, 2, 3] = True
    d = R.dilate(occ)
    assert d.sum() == 27 and d[1:4, 1:4, 2:5].all()
    d2 = R.dilate(occ, 2)
    assert d2.sum() == 4 * 5 * 5 and d2[0:4, 0:5, 1:6].all()
    np.testing.assert_array_equal(R.dilate(occ, 0), occ)
    occ[:] = False
    occ[3, 4, 5] = True
    assert R.dilate(occ).sum() == 8


@pytest.mark.parametrize('cells', [(1, 1, 1), (3, 5, 7), (4, 4, 2), (40, 33, 64), (5, 1, 13)])
def test_pack_unpack_layout(cells):
    rs = np.random.RandomState(sum(cells))
    occ = rs.rand(*cells) < 0.4
    w = R.pack(occ)
    assert w.dtype == np.int32 and w.shape == ((occ.size + 31) // 32,)
    np.testing.assert_array_equal(R.unpack(w, cells), occ)
    for l in rs.randint(0, occ.size, 20):                        # bit l & 31 of word l >> 5, z fastest
        ix, r = divmod(int(l), cells[1] * cells[2])
        iy, iz = divmod(r, cells[2])
        assert bool((int(w[l >> 5]) >> (l & 31)) & 1) == bool(occ[ix, iy, iz])
    if occ.size % 32:
        bad = w.copy()
        bad[-1] = np.int32(-1)
        with pytest.raises(AssertionError):
            R.unpack(bad, cells)


def test_cell_lookup_in_fp32():
    bmin, bmax, cells = (-1.0, 0.0, 2.0), (1.0, 3.0, 2.5), (4, 3, 5)
    pts = np.array([[-1.0, 0.0, 2.0],            # the lower corner is inside, cell (0, 0, 0)
                    [1.0, 1.0, 2.2],             # the upper face is outside (f == c)
                    [0.99, 2.99, 2.49],          # last cell
                    [-1.0001, 1.0, 2.2],
                    [np.nan, 1.0, 2.2], [0.0, np.inf, 2.2], [0.0, 1.0, -np.inf],
                    [0.25, 1.5, 2.25]], np.float32)
    inside, l = R.cell_of(pts, bmin, bmax, cells)
    np.testing.assert_array_equal(inside, [True, False, True, False, False, False, False, True])
    assert l[0] == 0 and l[2] == 4 * 3 * 5 - 1
    assert l[7] == (2 * 3 + 1) * 5 + 2
    occ = np.zeros(cells, bool)
    np.testing.assert_array_equal(R.keep(pts, bmin, bmax, cells, occ), ~inside)      # outside the box: always kept
    occ[2, 1, 2] = True
    assert R.keep(pts, bmin, bmax, cells, occ)[7]
    inv = R.inverse(bmin, bmax, cells)
    assert inv.dtype == np.float32
    np.testing.assert_array_equal(inv, np.array([2.0, 1.0, 10.0], np.float32))


# ---- the host side of occupancy.py ------------------------------------------------------------------------------------

def _grid(cells=(5, 3, 7), seed=0):
    occ = np.random.RandomState(seed).rand(*cells) < 0.5
    return OccupancyGrid((-1, -2, 0), (1, 2, 0.5), cells, R.pack(occ)), occ


def test_grid_fields_and_fraction():
    g, occ = _grid()
    assert g.cells == (5, 3, 7) and g.bmin.dtype == np.float32 and g.inv.dtype == np.float32
    np.testing.assert_array_equal(g.inv, R.inverse(g.bmin, g.bmax, g.cells))
    assert g.words.dtype == torch.int32 and g.words.shape == (4,)
    assert g.occupied_fraction() == pytest.approx(occ.mean())
    assert g.box() == [-1.0, -2.0, 0.0] + [float(v) for v in g.inv]
    assert g.stats['network_launches'] == 0


def test_save_load_round_trip(tmp_path):
    g, occ = _grid((40, 33, 64), seed=3)
    p = str(tmp_path / 'grid.npz')
    g.save(p)
    h = OccupancyGrid.load(p)
    assert h.cells == g.cells and torch.equal(h.words, g.words)
    for a in ('bmin', 'bmax', 'inv'):
        np.testing.assert_array_equal(getattr(h, a), getattr(g, a))
    np.testing.assert_array_equal(R.unpack(h.words.numpy(), h.cells), occ)
    with np.load(p) as d:
        assert sorted(d.files) == ['bmax', 'bmin', 'cells', 'inv', 'version', 'words']
    np.savez(str(tmp_path / 'other.npz'), words=g.words.numpy())
    with pytest.raises(ValueError):
        OccupancyGrid.load(str(tmp_path / 'other.npz'))


def test_constructor_value_errors():
    w = np.zeros(4, np.int32)
    ok = ((-1, -2, 0), (1, 2, 0.5), (5, 3, 7))
    OccupancyGrid(*ok, w)
    for bmin, bmax in [((0, 0, 0), (1, 1, 0)), ((0, 0, 0), (1, -1, 1)), ((0, 0), (1, 1)), ((0, 0, np.nan), (1, 1, 1)),
                       ((0, 0, 0), (1, np.inf, 1))]:
        with pytest.raises(ValueError):
            OccupancyGrid(bmin, bmax, ok[2], w)
    for cells in [(5, 3), (0, 3, 7), (5, 3, 513), (5, 3, 7, 1)]:
        with pytest.raises(ValueError):
            OccupancyGrid(ok[0], ok[1], cells, w)
    for words in [np.zeros(3, np.int32), np.zeros(5, np.int32), np.zeros(4, np.int64), np.zeros(4, np.float32),
                  np.zeros((2, 2), np.int32)]:
        with pytest.raises(ValueError):
            OccupancyGrid(*ok, words)
    with pytest.raises(ValueError):
        OccupancyGrid(*ok, w).lookup(np.zeros((3, 3), np.float32))              # not a tensor
    with pytest.raises(ValueError):
        OccupancyGrid(*ok, w).lookup(torch.zeros(3, 2))


def test_from_density_value_errors():
    lo, hi = (0, 0, 0), (1, 1, 1)
    s = torch.zeros(5, 5, 5)
    for kw in [dict(threshold=-1.0), dict(threshold=float('nan')), dict(threshold=float('inf')),
               dict(threshold=1.0, samples_per_cell=0), dict(threshold=1.0, samples_per_cell=9),
               dict(threshold=1.0, samples_per_cell=1.5), dict(threshold=1.0, samples_per_cell=3),      # 5 != 3 c + 1
               dict(threshold=1.0, dilate=-1), dict(threshold=1.0, dilate=0.5)]:
        with pytest.raises(ValueError):
            OccupancyGrid.from_density(s, lo, hi, **kw)
    with pytest.raises(ValueError):
        OccupancyGrid.from_density(s.numpy(), lo, hi, 1.0)
    with pytest.raises(ValueError):
        OccupancyGrid.from_density(torch.zeros(5, 5), lo, hi, 1.0)
    with pytest.raises(ValueError):
        OccupancyGrid.from_density(torch.zeros(5, 5, 1), lo, hi, 1.0)
    with pytest.raises(ValueError):
        OccupancyGrid.from_density(torch.zeros(514, 2, 2), lo, hi, 1.0)          # 513 cells
    with pytest.raises(ValueError):
        OccupancyGrid.from_density(s, lo, (1, 0, 1), 1.0)


def test_from_model_value_errors():
    net = torch.nn.Linear(1, 1)
    kw = {'network_fn': net, 'network_fine': None, 'network_query_fn': None}
    lo, hi = (0, 0, 0), (1, 1, 1)
    with pytest.raises(ValueError):
        OccupancyGrid.from_model(dict(kw, ndc=True), lo, hi)
    with pytest.raises(ValueError):
        OccupancyGrid.from_model(kw, lo, hi, networks=('medium',))
    with pytest.raises(ValueError):
        OccupancyGrid.from_model(kw, lo, hi, networks=())
    with pytest.raises(ValueError):
        OccupancyGrid.from_model(kw, lo, hi, cells=0)
    with pytest.raises(ValueError):
        OccupancyGrid.from_model(kw, lo, hi, samples_per_cell=0)
    with pytest.raises(ValueError):
        OccupancyGrid.from_model(kw, (0, 0, 0), (0, 1, 1), cells=4)
    with pytest.raises(ValueError):
        OccupancyGrid.from_model(kw, lo, hi, cells=512, samples_per_cell=2)      # 1025 points per axis: density_grid's limit
    with pytest.raises(ValueError):
        OccupancyGrid.from_model(kw, lo, hi, cells=4, threshold=-0.5)


# ---- render_rays refusals that need no device -------------------------------------------------------------------------

def _cpu_render_args():
    from mvip_nerf_amd.run_nerf_helpers import NeRF
    net = NeRF(D=8, W=256, input_ch=63, output_ch=5, skips=[4], input_ch_views=27, use_viewdirs=True)
    rows = torch.zeros(4, 11)
    rows[:, 5] = -1.0
    rows[:, 6], rows[:, 7] = 1.0, 2.0
    rows[:, 10] = -1.0

    def qfn(*a):
        raise AssertionError('the network must not be queried')
    return rows, net, qfn


def test_render_rays_refusals():
    rows, net, qfn = _cpu_render_args()
    g, _ = _grid()
    base = dict(N_samples=8, N_importance=8, network_fine=net, occupancy=g)
    with pytest.raises(ValueError, match='backward'):
        run.render_rays(rows, net, qfn, **base)                                   # autograd on, parameters require grad
    with torch.no_grad():
        with pytest.raises(ValueError, match='raw_noise_std'):
            run.render_rays(rows, net, qfn, raw_noise_std=1.0, **base)
        with pytest.raises(ValueError, match='sigma_loss'):
            run.render_rays(rows, net, qfn, sigma_loss=object(), **base)
        with pytest.raises(ValueError, match='OccupancyGrid'):
            run.render_rays(rows, net, qfn, **dict(base, occupancy='grid.npz'))
        with pytest.raises(ValueError, match='11 columns'):
            run.render_rays(rows[:, :8], net, qfn, **base)
    assert g.stats == {'samples_coarse': 0, 'kept_coarse': 0, 'samples_fine': 0, 'kept_fine': 0, 'network_launches': 0}


def test_default_is_off():
    import inspect
    assert inspect.signature(run.render_rays).parameters['occupancy'].default is None
    assert occupancy.DEFAULT_THRESHOLD >= 0


# ---- the C ABI: arguments are validated before the first HIP call -------------------------------------------------------

def test_entry_points_validate_arguments_without_a_device():
    import ctypes
    from mvip_nerf_amd import _lib
    lib = _lib.load()
    OK, EINVAL = 0, -1
    box = (ctypes.c_float * 6)(0, 0, 0, 1, 1, 1)
    cells = (ctypes.c_int * 3)(4, 4, 4)
    X = ctypes.c_void_p(4096)                                    # a non-null operand that is never dereferenced here
    A = ctypes.c_void_p(4100)                                    # ... and one that is not 16-byte aligned
    assert lib.mvip_occupancy_groups(0, 64) == 0 and lib.mvip_occupancy_groups(16, 64) == 1
    assert lib.mvip_occupancy_groups(17, 64) == 2 and lib.mvip_occupancy_groups(1, 0) == -1
    assert lib.mvip_occupancy_groups(-1, 64) == -1 and lib.mvip_occupancy_groups(2 ** 31 // 64, 64) == -1
    # build / dilate
    for args in [(None, 4, 4, 4, 1, 1.0, X, None), (X, 4, 4, 4, 1, 1.0, None, None), (X, 0, 4, 4, 1, 1.0, X, None),
                 (X, 4, 513, 4, 1, 1.0, X, None), (X, 4, 4, 4, 0, 1.0, X, None), (X, 4, 4, 4, 9, 1.0, X, None),
                 (X, 4, 4, 4, 1, -1.0, X, None), (X, 4, 4, 4, 1, float('nan'), X, None), (X, 4, 4, 4, 1, float('inf'), X, None)]:
        assert lib.mvip_occupancy_build(*args) == EINVAL, args
    for args in [(None, 4, 4, 4, X, None), (X, 4, 4, 4, None, None), (X, 4, 4, 4, X, None), (X, 4, 4, 0, A, None)]:
        assert lib.mvip_occupancy_dilate(*args) == EINVAL, args
    # count / emit / lookup: the empty call is MVIP_OK with null operands, a grid is always required
    assert lib.mvip_occupancy_count(None, None, 0, 64, box, cells, X, None, None, None, None, None) == OK
    assert lib.mvip_occupancy_emit(None, None, 0, 64, box, cells, X, None, 0, None, None, None, None) == OK
    assert lib.mvip_occupancy_emit(None, None, 8, 64, box, cells, X, None, 0, None, None, None, None) == OK       # K == 0
    assert lib.mvip_occupancy_lookup(None, 0, box, cells, X, None, None) == OK
    assert lib.mvip_occupancy_count(None, None, 8, 64, box, cells, X, None, None, None, None, None) == EINVAL     # null operands
    assert lib.mvip_occupancy_count(X, X, 8, 0, box, cells, X, X, X, None, None, None) == EINVAL                 # S < 1
    assert lib.mvip_occupancy_count(X, X, 0, 64, None, cells, X, X, X, None, None, None) == EINVAL
    assert lib.mvip_occupancy_count(X, X, 0, 64, box, None, X, X, X, None, None, None) == EINVAL
    assert lib.mvip_occupancy_count(X, X, 0, 64, box, cells, None, X, X, None, None, None) == EINVAL
    assert lib.mvip_occupancy_count(X, X, 0, 64, box, (ctypes.c_int * 3)(4, 0, 4), X, X, X, None, None, None) == EINVAL
    for bad in [(0, 0, 0, 1, 0, 1), (0, 0, 0, 1, -1, 1), (0, float('nan'), 0, 1, 1, 1), (0, 0, 0, float('inf'), 1, 1)]:
        assert lib.mvip_occupancy_lookup(None, 0, (ctypes.c_float * 6)(*bad), cells, X, None, None) == EINVAL, bad
    assert lib.mvip_occupancy_emit(X, X, 8, 64, box, cells, X, X, -1, X, X, X, None) == EINVAL
    assert lib.mvip_occupancy_emit(X, X, 8, 64, box, cells, X, X, 8 * 64 + 1, X, X, X, None) == EINVAL
    assert lib.mvip_occupancy_emit(X, X, 8, 64, box, cells, X, None, 5, X, X, X, None) == EINVAL
    assert lib.mvip_occupancy_lookup(None, 5, box, cells, X, X, None) == EINVAL
    assert lib.mvip_occupancy_lookup(X, -1, box, cells, X, X, None) == EINVAL
    # scatter
    assert lib.mvip_scatter_raw(None, None, 0, 0, None, None) == OK
    for args in [(X, X, 5, 4, X, None), (X, X, -1, 4, X, None), (X, X, 2, 4, None, None), (None, X, 2, 4, X, None),
                 (X, None, 2, 4, X, None), (X, X, 2, 4, A, None), (A, X, 2, 4, X, None), (None, None, 0, 4, None, None),
                 (X, X, 2, 2 ** 31, X, None)]:
        assert lib.mvip_scatter_raw(*args) == EINVAL, args
