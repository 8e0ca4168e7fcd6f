"""The restatement of the mesh-to-mesh distance (tests/mesh_distance_numpy.py) against analysis, and the host logic around the
kernels of csrc/mesh_distance.hip: the grid's cell choice, mesh.load_ply, the binding table, the argument checks that the C ABI
makes before any device call.  No GPU."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_distance_numpy as D                          # noqa: E402

F32 = np.float32
TRI_V = np.asarray([[0, 0, 0], [4, 0, 0], [0, 4, 0]], F32)
TRI_F = np.asarray([[0, 1, 2]], np.int32)

# (query, closest point, squared distance) for the triangle (0,0,0) (4,0,0) (0,4,0), worked out by hand
REGIONS = {
    'interior': ((1, 1, 3), (1, 1, 0), 9),
    'edge ab': ((2, -2, 1), (2, 0, 0), 5),
    'edge bc': ((4, 4, 1), (2, 2, 0), 9),
    'edge ca': ((-3, 2, 1), (0, 2, 0), 10),
    'vertex a': ((-1, -1, 2), (0, 0, 0), 6),
    'vertex b': ((6, -1, 1), (4, 0, 0), 6),
    'vertex c': ((-1, 6, 1), (0, 4, 0), 6),
}


@pytest.mark.parametrize('side', [1, -1])
@pytest.mark.parametrize('region', list(REGIONS))
def test_one_triangle_all_seven_regions_both_sides(region, side):
    p, q, d2 = REGIONS[region]
    p = np.asarray([[p[0], p[1], side * p[2]]], F32)
    face, point, dist, best = D.closest_point(p, TRI_V, TRI_F)
    assert face.tolist() == [0] and best.tolist() == [float(d2)]
    np.testing.assert_array_equal(point, np.asarray([q], F32))
    assert dist.dtype == F32 and dist[0] == F32(np.sqrt(np.float64(d2)))


def test_point_in_the_plane_inside_the_triangle_is_at_distance_zero():
    face, point, dist, _ = D.closest_point(np.asarray([[1, 2, 0], [0, 0, 0], [2, 2, 0]], F32), TRI_V, TRI_F)
    assert dist.tolist() == [0, 0, 0]
    np.testing.assert_array_equal(point, np.asarray([[1, 2, 0], [0, 0, 0], [2, 2, 0]], F32))


def test_degenerate_faces_are_their_segments_and_points():
    v = np.asarray([[0, 0, 0], [1, 0, 0], [2, 0, 0], [1, 1, 1]], F32)
    line, dot = np.asarray([[0, 1, 2]], np.int32), np.asarray([[3, 3, 3]], np.int32)
    face, point, dist, best = D.closest_point(np.asarray([[1, 1, 0], [3, 0, 1], [-2, 0, 0]], F32), v, line)
    assert best.tolist() == [1.0, 2.0, 4.0] and np.all(np.isfinite(dist))
    np.testing.assert_array_equal(point, np.asarray([[1, 0, 0], [2, 0, 0], [0, 0, 0]], F32))
    face, point, dist, best = D.closest_point(np.asarray([[1, 1, 3], [1, 1, 1]], F32), v, dot)
    assert best.tolist() == [4.0, 0.0] and dist.tolist() == [2.0, 0.0]
    np.testing.assert_array_equal(point, np.asarray([[1, 1, 1], [1, 1, 1]], F32))
    # among faces: the degenerate ones take part like any other, the lowest index wins a tie
    both = np.concatenate([dot, line, line])
    face, _, dist, _ = D.closest_point(np.asarray([[1, 1, 1], [1, -1, 0]], F32), v, both)
    assert face.tolist() == [0, 1] and dist.tolist() == [0.0, 1.0]


def test_non_finite_queries_give_minus_one_and_nan():
    pts = np.asarray([[np.nan, 0, 0], [1, 1, 3], [0, np.inf, 0], [0, 0, -np.inf]], F32)
    face, point, dist, _ = D.closest_point(pts, TRI_V, TRI_F)
    assert face.tolist() == [-1, 0, -1, -1] and dist[1] == 3
    assert np.all(np.isnan(dist[[0, 2, 3]])) and np.all(np.isnan(point[[0, 2, 3]]))


@pytest.mark.parametrize('k', [1, 2, 3, 5])
def test_samples_count_weights_and_centroid(k):
    rng = np.random.default_rng(7)
    v = rng.standard_normal((9, 3)).astype(F32)
    f = np.asarray([[0, 1, 2], [3, 4, 5], [6, 7, 8], [0, 4, 8], [1, 1, 2]], np.int32)              # the last has no area
    pts, fos, w = D.sample_faces(v, f, k)
    assert pts.shape == (k * k * len(f), 3) and pts.dtype == F32 and w.dtype == np.float64
    np.testing.assert_array_equal(fos, np.repeat(np.arange(len(f)), k * k))
    area = D.face_areas(v, f)
    assert area[-1] == 0 and np.all(area[:-1] > 0)
    for i in range(len(f)):
        # k^2 equal weights of two roundings each: the sum is within k^2 2^-52 of the area
        assert abs(w[fos == i].sum() - area[i]) <= k * k * 2.0 ** -52 * area[i]
    assert abs(w.sum() - area.sum()) <= len(w) * 2.0 ** -52 * area.sum()
    v64 = v.astype(np.float64)
    if k == 1:
        np.testing.assert_array_equal(pts, (((v64[f[:, 0]] + v64[f[:, 1]]) + v64[f[:, 2]]) / 3.0).astype(F32))
    # every sample lies in its own face: barycentrics positive, summing to one
    assert all(min(n) >= 1 and sum(n) == 3 * k for n in D.sample_order(k)) and len(set(D.sample_order(k))) == k * k
    face, _, dist, _ = D.closest_point(pts[fos == 0], v, f[:1])
    assert dist.max() <= 4 * 2.0 ** -24 * np.abs(v[f[0]]).max()                       # the fp32 rounding of the sample


def test_parallel_squares_give_one_eighth_everywhere():
    va, fa = D.square_mesh(4, 0.0)
    vb, fb = D.square_mesh(2, 0.125, flip=True)
    assert len(fa) == 32 and len(fb) == 8
    for (v0, f0), (v1, f1) in (((va, fa), (vb, fb)), ((vb, fb), (va, fa))):
        pts, _, _ = D.sample_faces(v0, f0, 3)
        _, point, dist, _ = D.closest_point(pts, v1, f1)
        assert np.all(dist == F32(0.125))
        np.testing.assert_array_equal(point[:, :2], pts[:, :2])
    rep = D.mesh_distance_metrics(va, fa, vb, fb, samples=3, thresholds=(0.2, 0.1))
    for d in (rep['a_to_b'], rep['b_to_a']):
        assert d['mean'] == d['rms'] == d['max'] == 0.125 and d['normal_consistency'] == 1.0 and abs(d['area'] - 1.0) < 1e-12
        assert d['within'] == [1.0, 0.0]
    assert rep['chamfer'] == rep['hausdorff'] == 0.125 and rep['normal_consistency'] == 1.0
    assert rep['fscore'] == [1.0, 0.0] and rep['precision'] == [1.0, 0.0] and rep['recall'] == [1.0, 0.0]


def test_nested_cubes_give_the_analytic_maximum():
    centre = (0.25, -0.5, 0.125)
    va, fa = D.cube_mesh(0.5, centre)
    vb, fb = D.cube_mesh(1.0, centre)                     # the same cube scaled by 2 about its centre
    rep = D.mesh_distance_metrics(va, fa, vb, fb, samples=4, thresholds=(0.5, 0.49))
    # every point of the inner cube's surface is exactly half an edge from the outer face in front of it
    assert rep['a_to_b']['max'] == 0.5 and rep['a_to_b']['mean'] == 0.5 and rep['a_to_b']['within'] == [1.0, 0.0]
    # the outer cube: 0.5 in front of the inner faces, up to sqrt(3) / 2 at the corners, which no sample reaches
    assert 0.5 < rep['b_to_a']['max'] < np.sqrt(3.0) / 2 and rep['b_to_a']['mean'] > 0.5
    assert rep['hausdorff'] == rep['b_to_a']['max'] and rep['a_to_b']['area'] == 6.0 and rep['b_to_a']['area'] == 24.0
    assert rep['a_to_b']['normal_consistency'] == 1.0                                  # parallel faces in front of each other


def test_report_of_the_package_equals_the_restatement_on_given_distances():
    """evaluate.mesh_distance_direction (the host half of evaluate.mesh_distance_metrics) against direction_report."""
    from mvip_nerf_amd import evaluate
    va, fa = D.cube_mesh(0.5)
    vb, fb = D.cube_mesh(0.75, (0.1, 0.0, -0.05))
    pts, fos, w = D.sample_faces(va, fa, 3)
    face, _, dist, _ = D.closest_point(pts, vb, fb)
    want = D.direction_report(dist, w, D.unit_normals(va, fa), fos, D.unit_normals(vb, fb), face, (0.3, 0.2))
    import torch
    na, nb = (evaluate._unit_face_normals(torch.from_numpy(v), torch.from_numpy(f)) for v, f in ((va, fa), (vb, fb)))
    assert evaluate.mesh_distance_direction(dist, w, na, fos, nb, face, (0.3, 0.2)) == want


def test_face_grid_cells_host_logic():
    from mvip_nerf_amd import ops
    box, cells = ops.mesh_face_grid_cells((-1, -1, -1), (1, 1, 1), 8000)
    assert cells == (20, 20, 20) and box[:3].tolist() == [-1, -1, -1] and box[3] == box[4] == box[5] == F32(10.0)
    box, cells = ops.mesh_face_grid_cells((0, 0, 0), (4, 2, 1), 64)                    # cubic cells on a non-cubic box
    assert cells == (8, 4, 2) and box[3] == box[4] == box[5] == F32(2.0)
    box, cells = ops.mesh_face_grid_cells((0, 0, 0.125), (1, 1, 0.125), 32)             # a flat mesh: one cell across, inv 1
    assert cells[2] == 1 and box[5] == 1.0 and cells[0] == cells[1] == 6
    assert ops.mesh_face_grid_cells((1, 2, 3), (1, 2, 3), 1)[1] == (1, 1, 1)
    assert ops.mesh_face_grid_cells((0, 0, 0), (1, 1, 1), 10 ** 9)[1] == (512, 512, 512)    # the stated maximum
    box, cells = ops.mesh_face_grid_cells((0, 0, 0), (1, 2, 4), 1, cells=(7, 3, 1))
    assert cells == (7, 3, 1) and box[3:].tolist() == [F32(7.0), F32(1.5), F32(0.25)]
    assert ops.mesh_face_grid_cells((0, 0, 0), (1, 1, 1), 5, cells=2)[1] == (2, 2, 2)
    # no cell narrower than 2^-20 of the coordinate magnitude
    assert ops.mesh_face_grid_cells((4096, 0, 0), (4096.5, 1, 1), 10 ** 9)[1][0] == 127
    for bad in (0, 513, (1, 2), (1, 0, 1)):
        with pytest.raises(ValueError, match='cells'):
            ops.mesh_face_grid_cells((0, 0, 0), (1, 1, 1), 5, cells=bad)
    with pytest.raises(ValueError, match='NaN or infinite'):
        ops.mesh_face_grid_cells((0, 0, 0), (1, np.inf, 1), 5)


def test_ply_round_trip_is_bit_equal(tmp_path):
    from mvip_nerf_amd import mesh
    rng = np.random.default_rng(3)
    v = rng.standard_normal((11, 3)).astype(F32)
    v[0, 0], v[1, 1] = -0.0, np.float32(1e-42)           # a negative zero and a denormal survive
    n = rng.standard_normal((11, 3)).astype(F32)
    f = rng.integers(0, 11, (7, 3)).astype(np.int32)
    c = rng.integers(0, 256, (11, 3)).astype(np.uint8)
    for colors in (c, None):
        a, b = str(tmp_path / 'a.ply'), str(tmp_path / 'b.ply')
        mesh.save_ply(a, mesh.Mesh(v, f, n, colors))
        m = mesh.load_ply(a)
        assert m.verts.dtype == F32 and m.faces.dtype == np.int32 and m.normals.dtype == F32
        assert m.verts.tobytes() == v.tobytes() and m.normals.tobytes() == n.tobytes() and m.faces.tobytes() == f.tobytes()
        assert (m.colors is None) if colors is None else (m.colors.tobytes() == c.tobytes())
        mesh.save_ply(b, m)
        assert open(a, 'rb').read() == open(b, 'rb').read()
    e = str(tmp_path / 'empty.ply')
    mesh.save_ply(e, mesh.Mesh(v[:0], f[:0], n[:0], None))
    m = mesh.load_ply(e)
    assert m.verts.shape == (0, 3) and m.faces.shape == (0, 3)
    open(e, 'ab').write(b'x')
    with pytest.raises(ValueError, match='bytes'):
        mesh.load_ply(e)
    open(e, 'wb').write(b'ply\nformat ascii 1.0\nend_header\n')
    with pytest.raises(ValueError, match='header'):
        mesh.load_ply(e)


NEW_SYMBOLS = ('mvip_mesh_distance_grid_count', 'mvip_mesh_distance_grid_scratch_words', 'mvip_mesh_distance_grid_fill',
               'mvip_mesh_distance_query', 'mvip_mesh_sample_faces')


def test_header_and_binding_table_hold_the_new_symbols():
    from mvip_nerf_amd import _lib
    from mvip_nerf_amd.csrc.build import SOURCES
    import test_abi
    assert 'mesh_distance.hip' in SOURCES
    header = test_abi.header_symbols()
    assert header == sorted(_lib.DECLARED_SYMBOLS)
    assert all(s in header for s in NEW_SYMBOLS)
    assert _lib.ABI_VERSION == 5


def test_the_abi_rejects_bad_arguments_before_any_device_call():
    from mvip_nerf_amd import _lib
    lib = _lib.load()
    box = (ctypes.c_float * 6)(0, 0, 0, 1, 1, 1)
    nanbox = (ctypes.c_float * 6)(0, 0, float('nan'), 1, 1, 1)
    zinv = (ctypes.c_float * 6)(0, 0, 0, 1, 0, 1)
    cells = (ctypes.c_int * 3)(2, 2, 2)
    big = (ctypes.c_int * 3)(513, 1, 1)
    one, null, st = 16, None, None                        # a non-NULL pointer that is never dereferenced: every call below is refused
    INT = 2 ** 31 - 1
    count = lambda **k: lib.mvip_mesh_distance_grid_count(*[k.get(n, d) for n, d in (
        ('verts', one), ('faces', one), ('V', 3), ('F', 1), ('box', box), ('cells', cells), ('off', one), ('total', one), ('flag', one))], st)
    for bad in (dict(F=0), dict(V=0), dict(F=-1), dict(F=INT), dict(V=INT + 1), dict(box=nanbox), dict(box=zinv), dict(box=None),
                dict(cells=big), dict(cells=None), dict(verts=null), dict(faces=null), dict(off=null), dict(total=null), dict(flag=null)):
        assert count(**bad) == -1, bad
    assert lib.mvip_mesh_distance_grid_scratch_words(-1, cells) == -1 and lib.mvip_mesh_distance_grid_scratch_words(INT + 1, cells) == -1
    assert lib.mvip_mesh_distance_grid_scratch_words(5, big) == -1 and lib.mvip_mesh_distance_grid_scratch_words(5, None) == -1
    assert lib.mvip_mesh_distance_grid_scratch_words(5, cells) == (5 + 8 + 2 + 1) // 2 * 2 + 15 + 2
    fill = lambda **k: lib.mvip_mesh_distance_grid_fill(*[k.get(n, d) for n, d in (
        ('verts', one), ('faces', one), ('V', 3), ('F', 1), ('box', box), ('cells', cells), ('off', one), ('P', 4), ('coff', one),
        ('cfaces', one), ('scratch', one))], st)
    for bad in (dict(F=0), dict(P=-1), dict(P=INT + 1), dict(box=nanbox), dict(cells=big), dict(verts=null), dict(off=null),
                dict(coff=null), dict(cfaces=null), dict(scratch=null)):
        assert fill(**bad) == -1, bad
    query = lambda **k: lib.mvip_mesh_distance_query(*[k.get(n, d) for n, d in (
        ('points', one), ('N', 2), ('verts', one), ('faces', one), ('V', 3), ('F', 1), ('box', box), ('cells', cells), ('coff', one),
        ('cfaces', one), ('P', 4), ('face', one), ('point', one), ('dist', one), ('stats', null))], st)
    for bad in (dict(F=0), dict(N=-1), dict(N=INT), dict(P=-1), dict(box=zinv), dict(cells=big), dict(points=null), dict(verts=null),
                dict(faces=null), dict(coff=null), dict(cfaces=null), dict(face=null), dict(point=null), dict(dist=null)):
        assert query(**bad) == -1, bad
    sample = lambda **k: lib.mvip_mesh_sample_faces(*[k.get(n, d) for n, d in (
        ('verts', one), ('faces', one), ('V', 3), ('F', 1), ('k', 2), ('points', one), ('fos', one), ('w', one), ('flag', one))], st)
    for bad in (dict(k=0), dict(k=-3), dict(k=1025), dict(F=-1), dict(V=-1), dict(V=0), dict(F=2 ** 20, k=1024), dict(verts=null),
                dict(faces=null), dict(points=null), dict(fos=null), dict(w=null), dict(flag=null)):
        assert sample(**bad) == -1, bad
