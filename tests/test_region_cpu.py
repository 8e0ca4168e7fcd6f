"""Regions without a GPU: the numpy restatement (tests/region_numpy.py) on hand-made cases, the host side of
mvip_nerf_amd/region.py (validation, save / load, carve, the box rule, every ValueError that needs no device), the C-ABI
declarations and the argument checks of the three entry points (the style of tests/test_abi_errors.py)."""
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import occupancy_numpy as R                              # noqa: E402
import region_numpy as G                                 # noqa: E402

from mvip_nerf_amd import _lib, region, run               # noqa: E402
from mvip_nerf_amd.occupancy import OccupancyGrid         # noqa: E402
from mvip_nerf_amd.region import Region                   # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ('mvip_region_mark', 'mvip_region_accumulate', 'mvip_region_lookup')


# ---- the C ABI ---------------------------------------------------------------------------------------------------------

def test_header_and_binding_table_declare_the_three_entry_points():
    txt = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'mvip_nerf.h')).read(), flags=re.S)
    declared = set(re.findall(r'\b(mvip_[a-z0-9_]+)\s*\(', txt))
    for name in SYMBOLS:
        assert name in declared and name in _lib.DECLARED_SYMBOLS, name
        assert hasattr(_lib.load(), name)
    assert _lib.load().mvip_abi_version() == 5                   # additive change


OK, EINVAL = 0, -1
P0 = None


def _grid_args(cells=(4, 4, 4), box=(0, 0, 0, 2, 2, 2)):
    import ctypes
    return (ctypes.c_float * 6)(*box), (ctypes.c_int * 3)(*cells)


def test_entry_point_argument_checks():
    """Before the first HIP call: a malformed call is MVIP_EINVAL, an empty call MVIP_OK, a null operand MVIP_EINVAL.
    `words` is checked for null only, so a non-null integer stands in for a device pointer; nothing is launched."""
    lib = _lib.load()
    box, cells = _grid_args()
    W = 64                                                        # a non-null address that is never dereferenced
    bad_cells = _grid_args(cells=(4, 0, 4))[1]
    big_cells = _grid_args(cells=(4, 513, 4))[1]
    bad_inv = _grid_args(box=(0, 0, 0, 2, 0, 2))[0]
    nan_box = _grid_args(box=(float('nan'), 0, 0, 2, 2, 2))[0]
    for b, c in ((box, bad_cells), (box, big_cells), (bad_inv, cells), (nan_box, cells), (None, cells), (box, None)):
        assert lib.mvip_region_mark(P0, 0, b, c, W, P0) == EINVAL
        assert lib.mvip_region_lookup(P0, 0, b, c, W, P0, P0) == EINVAL
        assert lib.mvip_region_accumulate(P0, P0, P0, 0, 64, b, c, W, P0, P0) == EINVAL
    # null words, negative counts, S < 1, B * S beyond int32
    assert lib.mvip_region_mark(P0, 0, box, cells, P0, P0) == EINVAL
    assert lib.mvip_region_mark(P0, -1, box, cells, W, P0) == EINVAL
    assert lib.mvip_region_lookup(P0, -1, box, cells, W, P0, P0) == EINVAL
    assert lib.mvip_region_accumulate(P0, P0, P0, -1, 64, box, cells, W, P0, P0) == EINVAL
    assert lib.mvip_region_accumulate(P0, P0, P0, 0, 0, box, cells, W, P0, P0) == EINVAL
    assert lib.mvip_region_accumulate(P0, P0, P0, 1 << 26, 64, box, cells, W, P0, P0) == EINVAL
    # empty calls
    assert lib.mvip_region_mark(P0, 0, box, cells, W, P0) == OK
    assert lib.mvip_region_lookup(P0, 0, box, cells, W, P0, P0) == OK
    assert lib.mvip_region_accumulate(P0, P0, P0, 0, 64, box, cells, W, P0, P0) == OK
    # well-formed shapes with null operands
    assert lib.mvip_region_mark(P0, 8, box, cells, W, P0) == EINVAL
    assert lib.mvip_region_lookup(P0, 8, box, cells, W, P0, P0) == EINVAL
    assert lib.mvip_region_accumulate(P0, P0, P0, 8, 64, box, cells, W, P0, P0) == EINVAL


# ---- the restatement ---------------------------------------------------------------------------------------------------

def test_inside_on_hand_made_points():
    bmin, bmax, cells = (-1.0, 0.0, 2.0), (1.0, 3.0, 2.5), (4, 3, 5)
    pts = np.array([[-1.0, 0.0, 2.0],            # the lower corner is in the box, cell (0, 0, 0)
                    [1.0, 1.0, 2.2],             # the upper face is outside (f == c)
                    [-0.5, 1.0, 2.25],           # on the face between cells 0 and 1 along x (and 0 and 1 along y): the upper ones
                    [-1.0001, 1.0, 2.2],
                    [np.nan, 1.0, 2.2], [0.0, np.inf, 2.2], [0.0, 1.0, -np.inf],
                    [0.25, 1.5, 2.25]], np.float32)
    none, full = np.zeros(cells, bool), np.ones(cells, bool)
    assert not G.inside(pts, bmin, bmax, cells, none).any()
    in_box = np.array([True, False, True, False, False, False, False, True])
    np.testing.assert_array_equal(G.inside(pts, bmin, bmax, cells, full), in_box)
    # inside is NOT keep: outside the box occupancy keeps, a region excludes
    np.testing.assert_array_equal(R.keep(pts, bmin, bmax, cells, none), ~in_box)
    one = none.copy()
    one[1, 1, 2] = True                                            # the cell of the face point: x in [-0.5, 0), y in [1, 2), z in [2.2, 2.3)
    np.testing.assert_array_equal(G.inside(pts, bmin, bmax, cells, one), [False, False, True, False, False, False, False, False])
    one[:] = False
    one[0, 1, 2] = one[1, 0, 2] = True                             # the cells below the faces do not hold it
    assert not G.inside(pts, bmin, bmax, cells, one).any()


def test_mark_and_accumulate_on_hand_made_cases():
    bmin, bmax, cells = (0, 0, 0), (4, 4, 4), (4, 4, 4)
    pts = np.array([[0.5, 0.5, 0.5], [3.5, 0.5, 2.5], [4.0, 1, 1], [np.nan, 1, 1], [0.5, 0.5, 0.9]], np.float32)
    reg = G.mark(pts, bmin, bmax, cells)
    assert reg.sum() == 2 and reg[0, 0, 0] and reg[3, 0, 2]
    again = G.mark(pts[:1], bmin, bmax, cells, reg)                # marking into cells already set changes nothing
    np.testing.assert_array_equal(again, reg)
    more = G.mark(np.array([[1.5, 1.5, 1.5]], np.float32), bmin, bmax, cells, reg)
    assert more.sum() == 3 and more[1, 1, 1] and reg.sum() == 2    # the input is not modified
    # one ray along x through y = z = 0.5: samples in cells 0..3, then outside
    ray = np.array([[[0.5, .5, .5], [1.5, .5, .5], [2.5, .5, .5], [3.5, .5, .5], [4.5, .5, .5]]], np.float32)
    w = np.array([[0.1, 0.2, 0.3, 0.25, np.nan]], np.float32)
    reg = np.zeros(cells, bool)
    reg[1, 0, 0] = reg[3, 0, 0] = True
    got, m = G.accumulate(ray, w, bmin, bmax, cells, reg)
    np.testing.assert_array_equal(m, [[False, True, False, True, False]])
    assert got[0] == np.float64(np.float32(0.2)) + np.float64(np.float32(0.25))     # the NaN outside is not read


def test_carve_is_the_complement_with_zero_tail_bits():
    cells = (5, 3, 7)                                              # 105 cells: 9 tail bits in the last word
    reg = np.random.RandomState(1).rand(*cells) < 0.3
    comp, words = G.carve(reg)
    np.testing.assert_array_equal(R.unpack(words, cells), ~reg)    # unpack asserts the tail bits are zero
    r = Region((0, 0, 0), (1, 1, 1), cells, R.pack(reg))
    grid = r.carve()
    assert isinstance(grid, OccupancyGrid) and grid.cells == cells
    # the two types share a base and nothing else: carve() and to() give each its own
    assert type(grid) is OccupancyGrid and type(r.to('cpu')) is Region and type(grid.to('cpu')) is OccupancyGrid
    np.testing.assert_array_equal(grid.words.numpy(), words)
    np.testing.assert_array_equal(grid.bmin, r.bmin)
    np.testing.assert_array_equal(grid.inv, r.inv)
    np.testing.assert_array_equal(r.words.numpy(), R.pack(reg))    # the region is not modified
    assert grid.occupied_fraction() == pytest.approx(1 - r.fraction())
    # a whole number of words: no tail
    reg = np.random.RandomState(2).rand(4, 4, 4) < 0.5
    np.testing.assert_array_equal(Region((0, 0, 0), (1, 1, 1), (4, 4, 4), R.pack(reg)).carve().words.numpy(), R.pack(~reg))
    # a sample inside the region is one the carved grid does not keep, and the other way round (in the box)
    pts = np.random.RandomState(3).uniform(-0.2, 1.2, (500, 3)).astype(np.float32)
    in_box, _ = R.cell_of(pts, (0, 0, 0), (1, 1, 1), (4, 4, 4))
    np.testing.assert_array_equal(G.inside(pts, (0, 0, 0), (1, 1, 1), (4, 4, 4), reg),
                                  ~R.keep(pts, (0, 0, 0), (1, 1, 1), (4, 4, 4), ~reg))
    assert (~in_box).any()


# ---- the host side of region.py ----------------------------------------------------------------------------------------

def _region(cells=(5, 3, 7), seed=0):
    reg = np.random.RandomState(seed).rand(*cells) < 0.5
    return Region((-1, -2, 0), (1, 2, 0.5), cells, R.pack(reg)), reg


def test_region_validation():
    r, reg = _region()
    assert r.cells == (5, 3, 7) and r.n_cells == 105 and r.words.dtype == torch.int32
    assert r.count() == int(reg.sum()) and r.fraction() == pytest.approx(reg.mean())
    np.testing.assert_array_equal(r.inv, R.inverse((-1, -2, 0), (1, 2, 0.5), (5, 3, 7)))
    assert len(r.box()) == 6
    assert Region((0, 0, 0), (1, 1, 1), 4, np.zeros(2, np.int32)).cells == (4, 4, 4)
    with pytest.raises(ValueError, match='cells'):
        Region((0, 0, 0), (1, 1, 1), (4, 0, 4), np.zeros(1, np.int32))
    with pytest.raises(ValueError, match='cells'):
        Region((0, 0, 0), (1, 1, 1), (4, 513, 4), np.zeros(1, np.int32))
    with pytest.raises(ValueError, match='below'):
        Region((0, 0, 0), (1, 0, 1), (4, 4, 4), np.zeros(2, np.int32))
    with pytest.raises(ValueError, match='finite'):
        Region((0, 0, 0), (1, np.inf, 1), (4, 4, 4), np.zeros(2, np.int32))
    with pytest.raises(ValueError, match='words'):
        Region((0, 0, 0), (1, 1, 1), (4, 4, 4), np.zeros(3, np.int32))
    with pytest.raises(ValueError, match='words'):
        Region((0, 0, 0), (1, 1, 1), (4, 4, 4), np.zeros(2, np.int64))
    with pytest.raises(ValueError, match='too thin'), np.errstate(over='ignore'):
        Region((0, 0, 0), (1, 1e-42, 1), (4, 4, 4), np.zeros(2, np.int32))
    assert r.to('cpu').words.device.type == 'cpu' and r.to('cpu') is not r


def test_save_load_round_trip_and_refusals(tmp_path):
    r, reg = _region()
    p = str(tmp_path / 'region.npz')
    r.save(p)
    q = Region.load(p)
    assert q.cells == r.cells and torch.equal(q.words, r.words)
    np.testing.assert_array_equal(q.bmin, r.bmin)
    np.testing.assert_array_equal(q.bmax, r.bmax)
    np.testing.assert_array_equal(q.inv, r.inv)
    with np.load(p) as d:
        assert str(d['kind']) == 'region' and sorted(d.files) == ['bmax', 'bmin', 'cells', 'inv', 'kind', 'version', 'words']
    # an occupancy grid's file is not a region: it means the opposite outside its box
    g = str(tmp_path / 'grid.npz')
    OccupancyGrid((-1, -2, 0), (1, 2, 0.5), (5, 3, 7), R.pack(reg)).save(g)
    with pytest.raises(ValueError, match='kind'):
        Region.load(g)
    OccupancyGrid.load(p)                                          # the other way round the extra key is ignored
    with np.load(p) as d:
        parts = dict(d)
    np.savez(str(tmp_path / 'kind.npz'), **dict(parts, kind=np.asarray('occupancy')))
    with pytest.raises(ValueError, match='kind'):
        Region.load(str(tmp_path / 'kind.npz'))
    np.savez(str(tmp_path / 'version.npz'), **dict(parts, version=np.asarray([99], np.int32)))
    with pytest.raises(ValueError, match='version'):
        Region.load(str(tmp_path / 'version.npz'))
    np.savez(str(tmp_path / 'inv.npz'), **dict(parts, inv=parts['inv'] * 2))
    with pytest.raises(ValueError, match='cell scale'):
        Region.load(str(tmp_path / 'inv.npz'))
    np.savez(str(tmp_path / 'missing.npz'), **{k: v for k, v in parts.items() if k != 'words'})
    with pytest.raises(ValueError, match='missing'):
        Region.load(str(tmp_path / 'missing.npz'))


@pytest.mark.parametrize('cells,dilate', [(64, 1), ((16, 8, 32), 0), (10, 2)])
def test_default_box_rule(cells, dilate):
    rs = np.random.RandomState(5)
    pts = rs.uniform(-3, 5, (1000, 3)) * [1.0, 0.1, 10.0]
    pts[:3] = [[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf]]
    finite = pts[3:]
    lo, hi = region.default_box(finite.min(0), finite.max(0), cells, dilate)
    wlo, whi = G.default_box(pts, (cells,) * 3 if np.isscalar(cells) else cells, dilate)
    assert lo.dtype == np.float32
    np.testing.assert_array_equal(lo, wlo)
    np.testing.assert_array_equal(hi, whi)
    # every point lies at least `dilate` cells from every face (the lowest in cell dilate + 1, the highest on the lower face
    # of cell c - dilate - 1, give or take fp32 rounding): no dilation round is clipped
    c = (cells,) * 3 if np.isscalar(cells) else cells
    _, l = R.cell_of(finite.astype(np.float32), lo, hi, c)
    in_box, _ = R.cell_of(finite.astype(np.float32), lo, hi, c)
    assert in_box.all()
    ix, iy, iz = l // (c[1] * c[2]), (l // c[2]) % c[1], l % c[2]
    for i, n in ((ix, c[0]), (iy, c[1]), (iz, c[2])):
        assert i.min() >= dilate and i.max() <= n - 1 - dilate
    reg = G.mark(finite.astype(np.float32), lo, hi, c)
    wide = R.dilate(np.pad(reg, dilate), dilate)                   # dilation in a box with room to spare
    assert wide.sum() == R.dilate(reg, dilate).sum()


def test_default_box_and_from_points_refusals():
    with pytest.raises(ValueError, match='inner cell'):
        region.default_box((0, 0, 0), (1, 1, 1), 4, 1)             # cells <= 2 (dilate + 1)
    with pytest.raises(ValueError, match='inner cell'):
        region.default_box((0, 0, 0), (1, 1, 1), (64, 2, 64), 0)
    region.default_box((0, 0, 0), (1, 1, 1), 5, 1)
    with pytest.raises(ValueError, match='zero extent'):
        region.default_box((0, 0, 0), (1, 0, 1), 64, 1)
    with pytest.raises(ValueError, match='no finite point'):
        region.default_box((np.inf,) * 3, (-np.inf,) * 3, 64, 1)
    with pytest.raises(ValueError, match='no finite point'):
        Region.from_points(torch.full((4, 3), float('nan')))
    with pytest.raises(ValueError, match='zero extent'):
        Region.from_points(torch.zeros((4, 3)))
    with pytest.raises(ValueError, match='inner cell'):
        Region.from_points(torch.rand((4, 3)), cells=4)
    with pytest.raises(ValueError, match='both'):
        Region.from_points(torch.rand((4, 3)), bmin=(0, 0, 0))
    with pytest.raises(ValueError, match='pts'):
        Region.from_points(np.zeros((4, 3)))
    with pytest.raises(ValueError, match='dilate'):
        Region.from_points(torch.rand((4, 3)), dilate=-1)


def test_from_masks_and_render_refusals_without_a_device():
    poses = torch.eye(4)[None, :3]
    masks = torch.ones((1, 4, 6), dtype=torch.bool)
    kw = dict(network_fn=None, network_query_fn=None, N_samples=8)
    with pytest.raises(ValueError, match='NDC'):
        Region.from_masks(dict(kw, ndc=True), (4, 6, 5.0), poses, masks, 1.0, 2.0)
    with pytest.raises(ValueError, match='raw_noise_std'):
        Region.from_masks(dict(kw, raw_noise_std=1.0), (4, 6, 5.0), poses, masks, 1.0, 2.0)
    with pytest.raises(ValueError, match='view directions'):
        Region.from_masks(dict(kw, use_viewdirs=False), (4, 6, 5.0), poses, masks, 1.0, 2.0)
    for bad in (masks[0], torch.ones((1, 6, 4), dtype=torch.bool), torch.ones((2, 4, 6), dtype=torch.bool)):
        with pytest.raises(ValueError, match='masks'):
            Region.from_masks(kw, (4, 6, 5.0), poses, bad, 1.0, 2.0)
    with pytest.raises(ValueError, match='min_weight'):
        Region.from_masks(kw, (4, 6, 5.0), poses, masks, 1.0, 2.0, min_weight=0.0)
    r, _ = _region()
    with pytest.raises(ValueError, match='region.Region'):
        region.propagate_masks(kw, (4, 6, 5.0), poses, r.carve(), 1.0, 2.0)
    rows = torch.zeros((4, 11))
    with pytest.raises(ValueError, match='region.Region'):
        run.render_rays(rows, None, None, 8, region=r.carve())     # an occupancy grid is not a region
    with pytest.raises(ValueError, match='11 columns'):
        run.render_rays(torch.zeros((4, 8)), None, None, 8, region=r)
