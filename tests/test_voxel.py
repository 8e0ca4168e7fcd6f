"""Mesh voxelisation on the GPU (csrc/mesh_voxel.hip) against its restatement tests/voxel_numpy.py: words, odd_columns and dropped
EQUAL, no tolerance, nothing excluded -- both are fp64 and integers; then what is built on it: mesh.voxelize, Region.from_mesh,
OccupancyGrid.from_mesh.  What the definition guarantees is checked on the restatement in tests/test_voxel_cpu.py."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_raycast_numpy as C                           # noqa: E402
import voxel_numpy as V                                  # noqa: E402

from mvip_nerf_amd import mesh, ops                      # noqa: E402
from mvip_nerf_amd.occupancy import OccupancyGrid        # noqa: E402
from mvip_nerf_amd.region import Region                  # noqa: E402

pytestmark = pytest.mark.gpu

F32, I32 = np.float32, np.int32
BOX1 = ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))
GRIDS = [(24, 20, 17), (1, 1, 1), (33, 1, 1), (5, 3, 70), (512, 2, 3)]
_cache = {}


def once(key, make):
    """a mesh or a reference, made once and left unchanged"""
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def dev(cuda, v, f):
    return torch.from_numpy(np.array(v, F32)).to(cuda).reshape(-1, 3), torch.from_numpy(np.array(f, I32)).to(cuda).reshape(-1, 3)


def reference(v, f, box, cells):
    """{axes: (words, odd, dropped)} for the four `axes`, and 'surface': (words, dropped)"""
    out = {'surface': V.surface(v, f, box, cells)}
    w, odd, dropped, per = V.solid(v, f, box, cells)
    out['majority'] = (w, odd, dropped)
    for a, name in enumerate(('x', 'y', 'z')):
        if dropped == 0:                                 # the same faces are walked: the single axis is the majority's own
            out[name] = (V.pack(per[a]), [odd[k] if k == a else 0 for k in range(3)], 0)
        else:
            out[name] = V.solid(v, f, box, cells, name)[:3]
    return out


def check(cuda, key, v, f, box, cells):
    ref = once(key, lambda: reference(v, f, box, cells))
    tv, tf = dev(cuda, v, f)
    words, dropped = ops.mesh_voxelize_surface(tv, tf, box, cells)
    assert words.dtype == torch.int32 and np.array_equal(words.cpu().numpy(), ref['surface'][0]), (key, 'surface')
    assert dropped == ref['surface'][1]
    for axes in V.AXES:
        words, odd, dropped = ops.mesh_voxelize_solid(tv, tf, box, cells, axes)
        assert np.array_equal(words.cpu().numpy(), ref[axes][0]), (key, axes)
        assert list(odd) == list(ref[axes][1]) and dropped == ref[axes][2], (key, axes, odd, dropped, ref[axes][1:])
    return ref


@pytest.mark.parametrize('cells', GRIDS, ids=lambda c: 'x'.join(map(str, c)))
@pytest.mark.parametrize('level', [2, 3])
def test_icosphere_equals_the_restatement(level, cells, cuda):
    v, f = once(('ico', level), lambda: C.icosphere(level, 0.8))
    assert len(f) == 20 * 4 ** level
    ref = check(cuda, ('ico', level, cells), v, f, V.grid_box(*BOX1, cells), cells)
    assert ref['majority'][2] == 0 and (ref['majority'][0] != 0).any()


def spanning_mesh():
    """four triangles that span the box among 200 tiny ones, in the same waves"""
    rng = np.random.default_rng(11)
    big = np.asarray([[(-0.9, -0.9, -0.7), (0.9, -0.8, 0.1), (0.0, 0.9, 0.8)], [(-0.95, 0.9, -0.9), (0.9, 0.95, 0.9), (0.1, -0.9, 0.0)],
                      [(0.9, -0.9, 0.9), (-0.9, 0.0, -0.9), (0.9, 0.9, -0.2)], [(-3.0, -2.0, 0.3), (3.0, -2.0, 0.31), (0.0, 4.0, 0.29)]])
    verts, at = [], {3: 0, 70: 1, 130: 2, 199: 3}
    for i in range(204):
        if i in at:
            verts.append(big[at[i]])
        else:
            c = rng.uniform(-0.9, 0.9, 3)
            verts.append(c + rng.uniform(-0.03, 0.03, (3, 3)))
    v = np.asarray(verts).reshape(-1, 3).astype(F32)
    return v, np.arange(len(v), dtype=I32).reshape(-1, 3)


def bad_faces_mesh():
    """the icosphere plus faces beyond the guard band (on x only, and on all axes), of zero area, repeating a vertex, with a NaN
    and with an infinite vertex, interleaved"""
    v, f = C.icosphere(2, 0.8)
    n = len(v)
    extra = np.asarray([(1e6, 0.1, 0.2), (0.5, 0.5, 0.5), (-0.5, 0.3, 0.1), (2e6, -3e6, 1e6), (0.0, 0.0, 0.0), (0.25, 0.25, 0.25),
                        (0.5, 0.5, 0.5), (np.nan, 0.0, 0.0), (0.0, np.inf, 0.0), (0.3, -0.2, 0.6), (3e38, 3e38, -3e38)], F32)
    more = np.asarray([(n, n + 1, n + 2), (n + 3, n + 1, n + 2), (n + 4, n + 5, n + 6), (n + 1, n + 1, n + 2), (n + 1, n + 2, n + 2),
                       (n + 7, n + 1, n + 2), (n + 1, n + 8, n + 9), (n + 9, n + 9, n + 9), (n + 10, n + 1, n + 9)], I32)
    faces = np.concatenate([f[:100], more[:4], f[100:250], more[4:], f[250:]]).astype(I32)
    return np.concatenate([v, extra]), faces


CASES = {
    'tie': lambda: V.tie_mesh(),
    'tie_flipped': lambda: V.tie_mesh(True),
    'lattice': lambda: C.lattice_mesh() + (V.grid_box((0, 0, 0), (4, 4, 4), (8, 8, 4)), (8, 8, 4)),
    'spanning': lambda: spanning_mesh() + (V.grid_box(*BOX1, GRIDS[0]), GRIDS[0]),
    'hangs_low': lambda: C.icosphere(1, 0.5, (-1.0, 0.1, -0.9)) + (V.grid_box(*BOX1, GRIDS[0]), GRIDS[0]),
    'hangs_high': lambda: C.icosphere(1, 0.5, (1.0, 0.1, 0.9)) + (V.grid_box(*BOX1, GRIDS[0]), GRIDS[0]),
    'outside': lambda: C.icosphere(1, 0.5, (3.0, -2.5, 0.25)) + (V.grid_box(*BOX1, GRIDS[0]), GRIDS[0]),
    'bad_faces': lambda: bad_faces_mesh() + (V.grid_box(*BOX1, GRIDS[0]), GRIDS[0]),
    'no_faces': lambda: (C.icosphere(0)[0], np.zeros((0, 3), I32), V.grid_box(*BOX1, (5, 3, 70)), (5, 3, 70)),
    'nothing': lambda: (np.zeros((0, 3), F32), np.zeros((0, 3), I32), V.grid_box(*BOX1, (5, 3, 70)), (5, 3, 70)),
}


@pytest.mark.parametrize('name', list(CASES))
def test_case_equals_the_restatement(name, cuda):
    v, f, box, cells = once(('case', name), CASES[name])
    ref = check(cuda, ('ref', name), v, f, box, cells)
    solid, odd, dropped = ref['majority']
    if name.startswith('tie') or name in ('hangs_low', 'outside'):
        assert odd == [0, 0, 0] and dropped == 0
    if name == 'lattice':                                # open sheets: the columns through them are odd
        assert odd[0] > 0 and odd[1] > 0 and dropped == 0
    if name == 'hangs_high':
        assert odd[0] > 0 and odd[2] > 0 and odd[1] == 0
    if name in ('no_faces', 'nothing', 'outside'):
        assert not solid.any() and not ref['surface'][0].any()
    if name == 'spanning':
        assert V.unpack(ref['surface'][0], cells).sum() > 500
    if name == 'bad_faces':
        # NaN, inf, 3e38 (its lattice coordinate is finite in fp64) and the two faces beyond the band; 'x' keeps the x-only one
        assert ref['surface'][1] == 2 and dropped == 5 and ref['x'][2] == 4 and ref['y'][2] == 5


def test_an_index_out_of_range_raises(cuda):
    v, f = C.icosphere(1)
    box, cells = V.grid_box(*BOX1, (8, 8, 8)), (8, 8, 8)
    for bad in (len(v), -1, 2 ** 31 - 1):
        g = f.copy()
        g[37, 1] = bad
        tv, tf = dev(cuda, v, g)
        with pytest.raises(ValueError, match='outside'):
            ops.mesh_voxelize_surface(tv, tf, box, cells)
        for axes in ('majority', 'y'):
            with pytest.raises(ValueError, match='outside'):
                ops.mesh_voxelize_solid(tv, tf, box, cells, axes)
    tv, tf = dev(cuda, np.zeros((0, 3), F32), f[:1])
    with pytest.raises(ValueError, match='outside'):
        ops.mesh_voxelize_solid(tv, tf, box, cells)


def test_argument_checks_of_the_ops(cuda):
    tv, tf = dev(cuda, *C.icosphere(0))
    box, cells = V.grid_box(*BOX1, (8, 8, 8)), (8, 8, 8)
    with pytest.raises(ValueError, match='axes'):
        ops.mesh_voxelize_solid(tv, tf, box, cells, 'w')
    for op in (ops.mesh_voxelize_surface, ops.mesh_voxelize_solid):
        for bad in ((0, 8, 8), (8, 513, 8), (8, 8), 'abc'):
            with pytest.raises(ValueError, match='cells'):
                op(tv, tf, box, bad)
        for bad in (box[:5], box[:3] + [1.0, 0.0, 1.0], box[:3] + [1.0, -1.0, 1.0], box[:3] + [float('inf'), 1.0, 1.0],
                    [float('nan')] + box[1:], box[:3] + [1e300, 1.0, 1.0]):
            with pytest.raises(ValueError, match='box'):
                op(tv, tf, bad, cells)
        with pytest.raises(ValueError, match='contiguous'):
            op(tv.repeat(1, 2)[:, ::2], tf, box, cells)
    with pytest.raises(ValueError, match='mode'):
        mesh.voxelize(mesh.Mesh(tv, tf, None, None), *BOX1, 8, mode='shell')
    with pytest.raises(ValueError, match='axes'):
        mesh.voxelize(mesh.Mesh(tv, tf, None, None), *BOX1, 8, axes='xy')


def test_face_order_and_repetition_leave_every_bit(cuda):
    v, f = once(('ico', 3), lambda: C.icosphere(3, 0.8))
    cells = GRIDS[0]
    box = V.grid_box(*BOX1, cells)
    v2, f2 = once(('case', 'spanning'), CASES['spanning'])[:2]
    f = np.concatenate([f, f2 + len(v)]).astype(I32)                      # with the wave path of both kernels in it
    v = np.concatenate([v, v2])
    tv, tf = dev(cuda, v, f)

    def run(faces):
        s, ds = ops.mesh_voxelize_surface(tv, faces, box, cells)
        w, odd, d = ops.mesh_voxelize_solid(tv, faces, box, cells)
        return s.cpu().numpy(), ds, w.cpu().numpy(), odd, d
    first = run(tf)
    perm = torch.from_numpy(np.random.default_rng(3).permutation(len(f))).to(cuda)
    side = torch.cuda.Stream()
    a = torch.randn(2048, 2048, device=cuda)
    again = run(tf)
    with torch.cuda.stream(side):                                         # a second stream keeps the device busy meanwhile
        for _ in range(20):
            a = (a @ a).clamp(-1, 1)
    busy = run(tf)
    shuffled = run(tf[perm].contiguous())
    torch.cuda.synchronize()
    for other in (again, busy, shuffled):
        assert np.array_equal(first[0], other[0]) and np.array_equal(first[2], other[2])
        assert first[1] == other[1] and first[3] == other[3] and first[4] == other[4]


def two_spheres(cuda):
    va, fa = C.icosphere(2, 0.3, (-0.5, 0.0, 0.0))
    vb, fb = C.icosphere(2, 0.3, (0.5, 0.1, 0.0))
    v, f = np.concatenate([va, vb]), np.concatenate([fa, fb + len(va)]).astype(I32)
    return mesh.Mesh(*dev(cuda, v, f), None, None), v, f


def test_region_and_occupancy_from_mesh(cuda, tmp_path):
    m, v, f = two_spheres(cuda)
    cells = (32, 32, 32)
    pts = torch.tensor([[-0.5, 0.0, 0.0], [0.5, 0.1, 0.0], [0.0, 0.0, 0.0], [0.0, 0.8, -0.8], [3.0, 0.0, 0.0]], device=cuda)
    plain = Region.from_mesh(m, *BOX1, cells=cells, dilate=0)
    box = V.grid_box(*BOX1, cells)
    want = V.surface(v, f, box, cells)[0] | V.solid(v, f, box, cells)[0]
    assert isinstance(plain, Region) and np.array_equal(plain.words.cpu().numpy(), want)
    assert plain.contains(pts).cpu().tolist() == [True, True, False, False, False]
    shell = Region.from_mesh(m, *BOX1, cells=cells, solid=False, dilate=0)
    assert np.array_equal(shell.words.cpu().numpy(), V.surface(v, f, box, cells)[0])
    assert shell.contains(pts).cpu().tolist() == [False] * 5 and 0 < shell.count() < plain.count()
    grown = Region.from_mesh(m, *BOX1, cells=cells)                        # dilate = 1
    assert torch.equal(grown.words, ops.occupancy_dilate(plain.words, cells)) and grown.count() > plain.count()
    carved = plain.carve()
    assert isinstance(carved, OccupancyGrid) and carved.lookup(pts).cpu().tolist() == [False, False, True, True, True]
    path = str(tmp_path / 'region.npz')
    plain.save(path)
    back = Region.load(path, cuda)
    assert torch.equal(back.words, plain.words) and back.cells == plain.cells and np.array_equal(back.inv, plain.inv)
    auto = Region.from_mesh(m, cells=48)                                   # default_box over the vertices; the gap is 11 cells
    assert auto.contains(pts).cpu().tolist() == [True, True, False, False, False]
    assert np.all(auto.bmin < v.min(0)) and np.all(auto.bmax > v.max(0))
    occ = OccupancyGrid.from_mesh(m, *BOX1, cells=cells, dilate=0)
    assert torch.equal(occ.words, plain.words) and occ.lookup(pts).cpu().tolist() == [True, True, False, False, True]
    occ1 = OccupancyGrid.from_mesh(m, *BOX1, cells=cells)
    assert torch.equal(occ1.words, grown.words)
    assert 'ONLY where the mesh is' in OccupancyGrid.from_mesh.__doc__


def test_voxelize_report_and_one_component(cuda):
    m, v, f = two_spheres(cuda)
    cells = (32, 28, 24)
    box = V.grid_box(*BOX1, cells)
    cell_volume = (2.0 / 32) * (2.0 / 28) * (2.0 / 24)
    for mode, axes in (('both', 'majority'), ('solid', 'z'), ('surface', 'majority')):
        grid, rep = mesh.voxelize(m, *BOX1, cells, mode=mode, axes=axes)
        s = V.surface(v, f, box, cells)[0]
        w, odd, _, _ = V.solid(v, f, box, cells, axes)
        want = {'both': s | w, 'solid': w, 'surface': s}[mode]
        assert np.array_equal(grid.words.cpu().numpy(), want)
        count = int(V.unpack(want, cells).sum())
        assert rep['count'] == count == grid.count() and rep['dropped'] == 0 and rep['cells'] == cells
        assert rep['odd_columns'] == (None if mode == 'surface' else odd) and (odd == [0, 0, 0])
        assert abs(rep['volume'] - count * cell_volume) <= 1e-12 * rep['volume']
    # the solid volume against the two polyhedra's: within the cells their surfaces touch (tests/test_voxel_cpu.py)
    _, rep = mesh.voxelize(m, *BOX1, cells, mode='solid')
    touched = int(V.unpack(V.surface(v, f, box, cells)[0], cells).sum())
    half = len(f) // 2
    centre = np.asarray((-0.5, 0.0, 0.0))
    exact = 2 * V.polyhedron_volume((v[:len(v) // 2] - centre).astype(F32), f[:half])
    assert abs(rep['volume'] - exact) <= touched * cell_volume
    one = mesh.keep_components(m, containing=torch.tensor([[0.5, 0.1, 0.0]]))
    assert one.faces.shape[0] == half
    r = Region.from_mesh(one, *BOX1, cells=32, dilate=0)
    pts = torch.tensor([[-0.5, 0.0, 0.0], [0.5, 0.1, 0.0]], device=cuda)
    assert r.contains(pts).cpu().tolist() == [False, True]
    c = V.centres(V.grid_box(*BOX1, (32, 32, 32)), (32, 32, 32))
    assert not V.unpack(r.words.cpu().numpy(), (32, 32, 32))[c[..., 0] < 0].any()
