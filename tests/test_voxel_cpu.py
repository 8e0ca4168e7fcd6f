"""The restatement of the mesh voxelisation (tests/voxel_numpy.py, the definition of csrc/mesh_voxel.hip) against first
principles, on the CPU: what the definition guarantees is derived here and checked on the restatement; tests/test_voxel.py then
asks the GPU for the same bits.

The bound all the solid checks share.  A vertex's raster coordinates are snapped to multiples of 2^-8 of a cell, so each moves by
at most 2^-9; the snapped triangle's point of equal barycentrics is within 2^-9 sqrt 2 < 2^-8 of a cell of the true one, across
the column and not along it.  A centre farther than 2^-8 of a cell from the surface of a closed mesh therefore gets the exact
inside / outside answer on every axis.  In world units the bound is H = 2^-8 x the largest cell edge, plus 2^-22 for the fp32
rounding of inv (relative 2^-24 on coordinates below 4)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_distance_numpy as D                          # noqa: E402
import mesh_raycast_numpy as C                           # noqa: E402
import voxel_numpy as V                                  # noqa: E402

F64 = np.float64
_cache = {}


def once(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def band(box, cells):
    edge = np.max(1.0 / np.asarray(box[3:], F64))
    return edge / 256.0 + 2.0 ** -22


BOX1 = ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))
CELLS = (24, 20, 17)


def ico2():
    def make():
        v, f = C.icosphere(2, 0.8)
        box = V.grid_box(*BOX1, CELLS)
        return v, f, box, V.solid(v, f, box, CELLS)
    return once('ico2', make)


def test_icosphere_columns_even_axes_agree_and_the_band_holds():
    v, f, box, (words, odd, dropped, per) = ico2()
    assert len(f) == 320 and dropped == 0
    assert odd == [0, 0, 0]
    r_in, r_out = V.radii(v, f)
    H = band(box, CELLS)
    r = np.linalg.norm(V.centres(box, CELLS), axis=-1)
    inside, outside = r < r_in - H, r > r_out + H
    assert inside.sum() > 1500 and outside.sum() > 4000 and (~inside & ~outside).sum() < 0.05 * r.size
    got = V.unpack(words, CELLS)
    for bits in (per[0], per[1], per[2], got):
        assert bits[inside].all() and not bits[outside].any()
    clear = inside | outside
    assert np.array_equal(per[0][clear], per[1][clear]) and np.array_equal(per[0][clear], per[2][clear])
    for name, a in (('x', 0), ('y', 1), ('z', 2)):
        w, o, d, _ = V.solid(v, f, box, CELLS, name)
        assert np.array_equal(w, V.pack(per[a])) and o == [0 if k != a else odd[a] for k in range(3)] and d == 0


@pytest.mark.parametrize('name', ['ico3', 'cube', 'nested', 'low', 'outside'])
def test_closed_meshes_have_no_odd_column(name):
    """every column of a closed mesh is even -- as long as the column does not END inside the mesh: a crossing beyond the last
    centre leaves no mark (test_a_column_that_ends_inside_the_mesh_is_odd), so the meshes here stay below the last centres"""
    if name == 'ico3':
        v, f = C.icosphere(3, 0.8)
    elif name == 'cube':
        v, f = D.cube_mesh(0.5)
    elif name == 'nested':
        v, f, _ = C.nested_spheres(2)
        v = (v * 0.8).astype(np.float32)
    elif name == 'low':
        v, f = C.icosphere(1, 0.5, (-1.0, 0.1, -0.9))                # hangs out of the low side on x and z: the k < 0 clamp
    else:
        v, f = C.icosphere(1, 0.5, (3.0, -2.5, 0.25))                # lies outside the box
    for cells in ((24, 20, 17), (7, 9, 70)):
        words, odd, dropped, _ = V.solid(v, f, V.grid_box(*BOX1, cells), cells)
        assert odd == [0, 0, 0] and dropped == 0
        assert (words != 0).any() == (name != 'outside')


def test_a_column_that_ends_inside_the_mesh_is_odd():
    """a sphere hanging out of the HIGH side of x: the columns along x whose last centre is inside it are the odd ones"""
    cells = (24, 20, 17)
    box = V.grid_box(*BOX1, cells)
    centre = np.asarray((1.0, 0.1, 0.0))
    v, f = C.icosphere(2, 0.5, centre)
    r_in, r_out = V.radii((v - centre).astype(np.float32), f)
    _, odd, dropped, per = V.solid(v, f, box, cells)
    assert dropped == 0 and odd[1] == 0 and odd[2] == 0
    r = np.linalg.norm(V.centres(box, cells)[-1] - centre, axis=-1)          # the last layer on x
    H = band(box, cells)
    assert int((r < r_in - H).sum()) <= odd[0] <= int((r <= r_out + H).sum()) and odd[0] > 0
    assert odd[0] == int(per[0][-1].sum())


def test_removed_face_changes_only_its_own_columns():
    v, f, box, (words, _, _, per) = ico2()
    gone = 7
    f1 = np.delete(f, gone, 0)
    words1, odd1, dropped1, per1 = V.solid(v, f1, box, CELLS)
    assert dropped1 == 0 and sum(odd1) > 0
    g = V.lattice(v, box)[f[gone]]
    lo, hi = g.min(0) - 2.0 ** -9, g.max(0) + 2.0 ** -9
    c = [np.arange(n, dtype=F64) + 0.5 for n in CELLS]
    within = [(c[a] >= lo[a]) & (c[a] <= hi[a]) for a in range(3)]
    box3 = within[0][:, None, None] & within[1][None, :, None] & within[2][None, None, :]
    changed_any = 0
    for a in range(3):
        b, cc = (a + 1) % 3, (a + 2) % 3
        changed = per[a] != per1[a]
        changed_any += int(changed.sum())
        shadow = np.ones(CELLS, bool)
        for k in (b, cc):
            shape = [1, 1, 1]
            shape[k] = CELLS[k]
            shadow &= within[k].reshape(shape)
        assert not (changed & ~shadow).any()
        # the mesh was closed: a column is odd now exactly where its last cell changed, i.e. where the removed face crossed it
        assert int((per[a].take(-1, axis=a) != per1[a].take(-1, axis=a)).sum()) == odd1[a]
    assert changed_any > 0                                        # a single axis leaks
    agreed = (per[0] == per[1]) & (per[1] == per[2])
    moved = V.unpack(words, CELLS) != V.unpack(words1, CELLS)
    assert not (moved & agreed & ~box3).any()                     # what the definition guarantees
    assert not (moved & ~box3).any()                              # and on this mesh nothing outside the box moves at all


def test_tie_mesh_either_winding_any_order():
    v, f, box, cells = V.tie_mesh()
    ref = V.solid(v, f, box, cells)
    assert ref[1] == [0, 0, 0] and ref[2] == 0
    c = [np.arange(n, dtype=F64) + 0.5 for n in cells]
    lo, hi = (1.5, 1.5, 1.5), (5.5, 4.5, 3.5)
    strictly_in = np.ones(cells, bool)
    strictly_out = np.zeros(cells, bool)
    for a in range(3):
        shape = [1, 1, 1]
        shape[a] = cells[a]
        strictly_in &= ((c[a] > lo[a]) & (c[a] < hi[a])).reshape(shape)
        strictly_out |= ((c[a] < lo[a]) | (c[a] > hi[a])).reshape(shape)
    for bits in (ref[3][0], ref[3][1], ref[3][2], V.unpack(ref[0], cells)):
        assert bits[strictly_in].all() and not bits[strictly_out].any()
    rng = np.random.default_rng(5)
    for flip in (False, True):
        vv, ff, _, _ = V.tie_mesh(flip)
        for _ in range(3):
            got = V.solid(vv, ff[rng.permutation(len(ff))], box, cells)
            assert np.array_equal(got[0], ref[0]) and got[1] == [0, 0, 0]
            for a in range(3):
                assert np.array_equal(got[3][a], ref[3][a])


def surface_cases():
    v, f = C.icosphere(2, 0.8)
    yield 'icosphere', v, f, V.grid_box(*BOX1, CELLS), CELLS
    v, f = C.lattice_mesh()
    for cells in ((4, 4, 4), (8, 8, 4), (16, 16, 16)):
        yield f'lattice{cells}', v, f, V.grid_box((0, 0, 0), (4, 4, 4), cells), cells
    v, f = D.cube_mesh(0.5)
    yield 'cube', v, f, V.grid_box(*BOX1, (8, 8, 8)), (8, 8, 8)


def test_surface_holds_every_sample_of_every_face():
    for name, v, f, box, cells in surface_cases():
        words, dropped = V.surface(v, f, box, cells)
        bits = V.unpack(words, cells)
        pts, _, _ = D.sample_faces(v, f, 6)
        assert len(pts) == 36 * len(f) and dropped == 0
        ijk, inside = V.cell_of(pts, box, cells)
        assert inside.sum() > 0.9 * len(pts), name
        hit = bits[ijk[:, 0], ijk[:, 1], ijk[:, 2]]
        assert int((inside & ~hit).sum()) == 0, name
        assert bits.sum() < 0.5 * bits.size or name.startswith('lattice'), name    # conservative, not everything


def test_voxel_volume_of_the_icosphere():
    """|voxel volume - exact volume| <= (cells the surface touches) x cell volume: a cell the surface does not touch lies wholly
    on one side and its centre is half a cell from the surface, beyond the 2^-8 band, so its bit is exact and it contributes its
    whole volume or nothing to both; a cell within the band is touched, and the conservative surface set holds every touched cell."""
    cells = (64, 64, 64)
    v, f = C.icosphere(3, 0.8)
    box = V.grid_box(*BOX1, cells)
    words, odd, dropped, _ = V.solid(v, f, box, cells)
    assert odd == [0, 0, 0] and dropped == 0
    solid = V.unpack(words, cells)
    surf = V.unpack(V.surface(v, f, box, cells)[0], cells)
    r_in, r_out = V.radii(v, f)
    r = np.linalg.norm(V.centres(box, cells), axis=-1)
    H = band(box, cells)
    in_band = (r >= r_in - H) & (r <= r_out + H)
    assert not (in_band & ~surf).any()                            # the band lies inside the surface set
    cell_volume = float(np.prod(1.0 / np.asarray(box[3:], F64)))
    exact = V.polyhedron_volume(v, f)
    assert abs(exact - 4.0 / 3.0 * np.pi * 0.8 ** 3) < 0.02 * exact
    bound = int((surf | in_band).sum()) * cell_volume
    assert abs(int(solid.sum()) * cell_volume - exact) <= bound
    assert bound < 0.25 * exact                                   # the bound says something
