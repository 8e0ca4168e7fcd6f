"""Connected components on the GPU (csrc/components.hip; ops.grid_pack / grid_components / grid_select,
BitGrid.keep_components, mesh.remove_floaters) against the numpy restatement (tests/components_numpy.py).  Labels, sizes,
first indices and selected words are integers: every comparison is for equality."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import components_numpy as C                             # noqa: E402
import occupancy_numpy as R                              # noqa: E402

from mvip_nerf_amd import mesh, ops                       # noqa: E402
from mvip_nerf_amd.occupancy import OccupancyGrid         # noqa: E402
from mvip_nerf_amd.region import Region                   # noqa: E402

pytestmark = pytest.mark.gpu

BOX = ((-1.5, -1.2, -4.3), (1.5, 1.2, -0.7))
SNAKES = {(17, 17, 40): 3320, (9, 9, 37): 949, (5, 7, 33): 407}
# (shape, p, connectivity, components, cells of the largest): counted with scipy.ndimage.label
BIG = [((64, 64, 64), 0.34, 6, 11729, 56481), ((64, 64, 64), 0.12, 26, 2348, 25110), ((40, 33, 64), 0.34, 6, 3727, 17208)]

_reference = {}


def N(t):
    return t.detach().cpu().numpy()


def random_bits(shape, p=0.5):
    return np.random.RandomState(7).rand(*shape) < p


def reference(key, bits, connectivity):
    """The restatement's (labels, sizes, first), computed once per case and never modified."""
    k = (key, connectivity)
    if k not in _reference:
        _reference[k] = C.components(bits, connectivity)
        for a in _reference[k]:
            a.setflags(write=False)
    return _reference[k]


def run_components(bits, connectivity, cuda):
    labels, sizes, first = ops.grid_components(torch.from_numpy(C.pack(bits)).to(cuda), bits.shape, connectivity)
    assert labels.dtype == sizes.dtype == first.dtype == torch.int32 and tuple(labels.shape) == bits.shape
    return N(labels), N(sizes), N(first)


def check(key, bits, connectivity, cuda):
    want = reference(key, bits, connectivity)
    got = run_components(bits, connectivity, cuda)
    for name, g, w in zip(('labels', 'sizes', 'first'), got, want):
        assert g.shape == w.shape and np.array_equal(g, w), name
    return got


# ---- labelling -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('connectivity', [6, 26])
@pytest.mark.parametrize('shape', [(5, 7, 33), (3, 4, 31), (1, 1, 70), (9, 1, 1), (1, 1, 1)])
def test_random_shapes_equal_restatement(shape, connectivity, cuda):
    check(('random', shape), random_bits(shape), connectivity, cuda)


def test_opposite_corners(cuda):
    bits = np.zeros((2, 2, 2), bool)
    bits[0, 0, 0] = bits[1, 1, 1] = True
    assert list(check('corners', bits, 6, cuda)[1]) == [1, 1]
    assert list(check('corners', bits, 26, cuda)[1]) == [2]


@pytest.mark.parametrize('connectivity', [6, 26])
def test_row_wrap(connectivity, cuda):
    bits = np.zeros((2, 3, 5), bool)
    bits[0, 0, 4] = bits[0, 1, 0] = True                  # linear indices 4 and 5: adjacent numbers, cells apart
    labels, sizes, first = check('wrap', bits, connectivity, cuda)
    assert list(sizes) == [1, 1] and list(first) == [4, 5]


@pytest.mark.parametrize('connectivity', [6, 26])
@pytest.mark.parametrize('shape', list(SNAKES))
def test_one_long_component(shape, connectivity, cuda):
    bits = C.snake(shape)
    labels, sizes, first = check(('snake', shape), bits, connectivity, cuda)
    assert list(sizes) == [SNAKES[shape]] and list(first) == [0]
    assert np.array_equal(labels, bits.astype(np.int32))


@pytest.mark.parametrize('shape,p,connectivity,count,largest', BIG)
def test_many_workgroups(shape, p, connectivity, count, largest, cuda):
    labels, sizes, first = check(('big', shape, p), random_bits(shape, p), connectivity, cuda)
    assert len(sizes) == count and sizes.max() == largest
    assert np.all(np.diff(first) > 0)


@pytest.mark.parametrize('connectivity', [6, 26])
def test_edge_grids(connectivity, cuda):
    for shape in ((5, 7, 33), (64, 64, 64)):
        n = int(np.prod(shape))
        labels, sizes, first = run_components(np.ones(shape, bool), connectivity, cuda)
        assert np.all(labels == 1) and list(sizes) == [n] and list(first) == [0]
        labels, sizes, first = run_components(np.zeros(shape, bool), connectivity, cuda)
        assert not labels.any() and sizes.shape == (0,) and first.shape == (0,)
    # no component: the select launch is skipped, the words are zero
    words = ops.grid_select(torch.zeros((5, 7, 33), device=cuda, dtype=torch.int32), torch.zeros(1, device=cuda, dtype=torch.uint8))
    assert words.dtype == torch.int32 and not N(words).any() and words.shape == (C.n_words(5 * 7 * 33),)


def test_reproducible(cuda):
    shape, p, conn = BIG[0][:3]
    words = torch.from_numpy(C.pack(random_bits(shape, p))).to(cuda)
    a = ops.grid_components(words, shape, conn)
    b = ops.grid_components(words, shape, conn)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


# ---- pack / select ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('n', [0, 1, 63, 64, 65, 1000, 5 * 7 * 33, 70001])
def test_pack_equals_comparison(n, cuda):
    rs = np.random.RandomState(n)
    v = rs.randn(n).astype(np.float32)
    thr = np.float32(0.25)
    if n >= 63:
        v[:6] = [np.nan, np.inf, -np.inf, thr, np.nextafter(thr, np.float32(0)), np.nextafter(thr, np.float32(1))]
        v[-1] = thr
    words = ops.grid_pack(torch.from_numpy(v).to(cuda), float(thr))
    assert words.dtype == torch.int32
    with np.errstate(invalid='ignore'):
        want = v >= thr
    assert np.array_equal(C.unpack(N(words), (n,)), want)          # unpack asserts the tail bits are zero
    assert np.array_equal(N(words), C.pack_values(v, thr))
    if n >= 63:
        assert list(want[:6]) == [False, True, False, True, False, True]


@pytest.mark.parametrize('connectivity', [6, 26])
@pytest.mark.parametrize('shape', [(5, 7, 33), (3, 4, 31), (1, 1, 70), (40, 33, 64)])
def test_select_equals_restatement(shape, connectivity, cuda):
    bits = random_bits(shape, 0.34)
    labels, sizes, first = reference(('select', shape), bits, connectivity)
    rs = np.random.RandomState(3)
    keep = np.concatenate([[0], rs.rand(len(sizes)) < 0.5]).astype(np.uint8)
    got = ops.grid_select(torch.from_numpy(labels.copy()).to(cuda), torch.from_numpy(keep).to(cuda))
    assert np.array_equal(N(got), C.select(labels, keep))
    assert np.array_equal(C.unpack(N(got), shape), keep.astype(bool)[labels])


# ---- BitGrid.keep_components -------------------------------------------------------------------------------------------------

CELLS = (40, 33, 64)


def cell_centres(cells_l):
    """Centres of linear cells, fp64 -> fp32 (a centre is half a cell from every face: no rounding can move it out)."""
    lo, hi = np.float64(BOX[0]), np.float64(BOX[1])
    l = np.asarray(cells_l, np.int64)
    ijk = np.stack([l // (CELLS[1] * CELLS[2]), l // CELLS[2] % CELLS[1], l % CELLS[2]], -1)
    return (lo + (ijk + 0.5) * (hi - lo) / np.float64(CELLS)).astype(np.float32)


@pytest.mark.parametrize('cls', [OccupancyGrid, Region])
def test_keep_components(cls, cuda):
    bits = random_bits(CELLS, 0.34)
    labels, sizes, first = reference(('big', CELLS, 0.34), bits, 6)
    grid = cls(BOX[0], BOX[1], CELLS, torch.from_numpy(C.pack(bits)).to(cuda))
    got = grid.components(6)
    assert np.array_equal(N(got[0]), labels) and np.array_equal(N(got[1]), sizes) and np.array_equal(N(got[2]), first)
    big = int(np.argmax(sizes)) + 1
    single = int(np.flatnonzero(sizes == 1)[0]) + 1
    pts = cell_centres([np.flatnonzero(labels.reshape(-1) == big)[5], first[single - 1]])
    pts = np.concatenate([pts, [[9.0, 9.0, 9.0]], cell_centres(np.flatnonzero(~bits.reshape(-1))[:1])]).astype(np.float32)
    cases = [(dict(largest=1), None), (dict(largest=3), None), (dict(min_cells=2), None), (dict(containing=torch.from_numpy(pts).to(cuda)), [big, single]),
             (dict(largest=3, min_cells=100), None), (dict(min_cells=50, containing=pts), [big, single])]
    for kw, lab in cases:
        out = grid.keep_components(**kw)
        keep = C.keep_table(sizes, first, kw.get('largest'), kw.get('min_cells'), lab)
        assert type(out) is cls and out.cells == grid.cells, kw
        assert np.array_equal(out.bmin, grid.bmin) and np.array_equal(out.bmax, grid.bmax) and np.array_equal(out.inv, grid.inv)
        assert np.array_equal(N(out.words), C.select(labels, keep)), kw
        assert out.count() == int(sizes[keep[1:] != 0].sum()), kw
    assert torch.equal(grid.words, torch.from_numpy(C.pack(bits)).to(cuda))         # the grid itself is unchanged
    # a dropped cell's centre: no longer occupied / inside; a kept cell's centre still is
    out = grid.keep_components(largest=1)
    probe = torch.from_numpy(cell_centres([first[single - 1], first[big - 1]])).to(cuda)
    ask = out.contains if cls is Region else out.lookup
    before = grid.contains if cls is Region else grid.lookup
    assert N(before(probe)).tolist() == [True, True] and N(ask(probe)).tolist() == [False, True]
    at_26 = grid.keep_components(largest=1, connectivity=26)
    want = C.components(bits, 26)
    assert np.array_equal(N(at_26.words), C.select(want[0], C.keep_table(want[1], want[2], largest=1)))


# ---- meshes ----------------------------------------------------------------------------------------------------------------

MESH_SHAPE = (48, 40, 36)
THR = 1.0
SPECKS = [(3, 3, 3), (44, 5, 30), (5, 35, 5), (40, 36, 4), (2, 20, 33)]


def mesh_field():
    """sigma on a 48 x 40 x 36 lattice of [-1, 1]^3: a ball of radius 0.5 at the origin, one of radius 0.15 at
    (0.7, 0.6, 0.5), and five isolated lattice points above the threshold, well away from both."""
    ax = [np.linspace(-1, 1, n) for n in MESH_SHAPE]
    X, Y, Z = np.meshgrid(*ax, indexing='ij')
    d0 = np.sqrt(X ** 2 + Y ** 2 + Z ** 2)
    d1 = np.sqrt((X - 0.7) ** 2 + (Y - 0.6) ** 2 + (Z - 0.5) ** 2)
    g = np.maximum(THR + (0.5 - d0) * 4, THR + (0.15 - d1) * 4).astype(np.float32)
    for s in SPECKS:
        assert g[s] < THR - 0.5 and min(d0[s] - 0.5, d1[s] - 0.15) > 0.25
        g[s] = 3.0
    return g


def directed_edges_paired(faces):
    """Closed and consistently oriented: every directed edge (a, b) of a face occurs once, and so does (b, a)."""
    e = np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]]).astype(np.int64)
    fwd = e[:, 0] * (e.max() + 1) + e[:, 1]
    rev = e[:, 1] * (e.max() + 1) + e[:, 0]
    return len(np.unique(fwd)) == len(fwd) and np.array_equal(np.sort(fwd), np.sort(rev))


def test_mesh_floaters(cuda):
    g = mesh_field()
    grid = torch.from_numpy(g).to(cuda)
    lo, hi = (-1, -1, -1), (1, 1, 1)
    v0, f0, n0 = (N(t) for t in mesh.marching_cubes(grid, THR, lo, hi))
    labels, sizes, first = C.components(g >= THR, 6)
    assert sorted(sizes)[:5] == [1] * 5 and len(sizes) == 7

    cleaned = mesh.remove_floaters(grid, THR, largest=1)
    assert cleaned.dtype == torch.float32 and cleaned.shape == grid.shape
    main = labels == int(np.argmax(sizes)) + 1
    assert np.array_equal(N(cleaned), np.where(main | (labels == 0), g, np.float32(0)))
    assert torch.equal(grid, torch.from_numpy(g).to(cuda))                              # the input is not modified
    v1, f1, n1 = (N(t) for t in mesh.marching_cubes(cleaned, THR, lo, hi))
    near = np.linalg.norm(v0.astype(np.float64), axis=1) < 0.6
    assert 0 < near.sum() < len(v0)
    assert np.array_equal(v1.view(np.uint32), v0[near].view(np.uint32))                  # in order, bit for bit
    assert len(f1) == int(near[f0].all(1).sum()) and not (near[f0].any(1) & ~near[f0].all(1)).any()
    renumber = np.cumsum(near) - 1
    assert np.array_equal(f1, renumber[f0[near[f0].all(1)]])
    assert directed_edges_paired(f1)

    # min_points = 2 drops the five specks and keeps both balls
    v2, f2, _ = (N(t) for t in mesh.marching_cubes(mesh.remove_floaters(grid, THR, min_points=2), THR, lo, hi))
    speck_pts = np.stack([np.linspace(-1, 1, n)[[s[a] for s in SPECKS]] for a, n in enumerate(MESH_SHAPE)], -1)
    far = np.min(np.linalg.norm(v0[:, None, :].astype(np.float64) - speck_pts[None], axis=2), axis=1) > 0.1
    assert far.sum() == len(v0) - 6 * len(SPECKS)
    assert np.array_equal(v2.view(np.uint32), v0[far].view(np.uint32)) and len(f2) == len(f0) - 8 * len(SPECKS)
    assert directed_edges_paired(f2) and len(v2) > len(v1)
    both = mesh.remove_floaters(grid, THR, largest=2, min_points=2)
    assert torch.equal(both, mesh.remove_floaters(grid, THR, min_points=2))


def test_extract_mesh_default_is_unfiltered(cuda):
    """extract_mesh with largest = min_points = None takes today's path: the lattice reaches marching cubes as it is, and
    the tensors are those of the unfiltered call, bit for bit; with largest=1 they are those of the cleaned lattice."""
    g = torch.from_numpy(mesh_field()).to(cuda)
    seen = []
    real_grid, real_rf = mesh.density_grid, mesh.remove_floaters
    mesh.density_grid = lambda *a, **k: g
    mesh.remove_floaters = lambda *a, **k: seen.append((a[2:], k)) or real_rf(*a, **k)
    try:
        plain = mesh.extract_mesh({}, (-1, -1, -1), (1, 1, 1), resolution=MESH_SHAPE, threshold=THR, colors=False)
        assert not seen
        kept = mesh.extract_mesh({}, (-1, -1, -1), (1, 1, 1), resolution=MESH_SHAPE, threshold=THR, colors=False, largest=1)
        assert seen == [((1, None), {'connectivity': 6})]
    finally:
        mesh.density_grid, mesh.remove_floaters = real_grid, real_rf
    want = mesh.marching_cubes(g, THR, (-1, -1, -1), (1, 1, 1))
    for a, b in zip(plain[:3], want):
        assert torch.equal(a, b)
    assert plain.colors is None
    want = mesh.marching_cubes(mesh.remove_floaters(g, THR, largest=1), THR, (-1, -1, -1), (1, 1, 1))
    for a, b in zip(kept[:3], want):
        assert torch.equal(a, b) and a.shape[0] > 0
