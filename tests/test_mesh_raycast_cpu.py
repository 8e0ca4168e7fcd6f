"""The restatement of mesh ray casting (tests/mesh_raycast_numpy.py) against hand-computed rays and analysis -- one triangle,
ties, watertightness on an icosphere, the Fibonacci set, openness of nested spheres -- and the host logic around the kernels of
csrc/mesh_raycast.hip: the binding table, the argument checks that the C ABI makes before any device call.  No GPU."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_raycast_numpy as C                           # noqa: E402

F32, F64, I32 = np.float32, np.float64, np.int32
INF = np.inf
TRI_V = np.asarray([[0, 0, 0], [4, 0, 0], [0, 4, 0]], F32)
TRI_F = np.asarray([[0, 1, 2]], I32)


def one(o, d, tmin=0.0, tmax=INF, verts=TRI_V, faces=TRI_F, skip=None):
    face, t, bary, t64 = C.cast_rays(np.asarray([o], F32), np.asarray([d], F32), tmin, tmax, verts, faces,
                                     skip=None if skip is None else np.asarray([skip]))
    assert face.dtype == I32 and t.dtype == F32 and bary.dtype == F32 and t64.dtype == F64
    return int(face[0]), float(t[0]), bary[0].tolist(), float(t64[0])


# (origin, direction, t, (weight of b, weight of c)) for the triangle (0,0,0) (4,0,0) (0,4,0), worked out by hand
HITS = {
    'interior': ((1, 1, 3), (0, 0, -1), 3.0, (0.25, 0.25)),
    'interior, oblique': ((0, 0, 2), (1, 1, -1), 2.0, (0.5, 0.5)),          # lands on the edge bc at (2, 2, 0)
    'interior, scaled direction': ((1, 2, 8), (0, 0, -4), 2.0, (0.25, 0.5)),
    'edge ab': ((2, 0, 5), (0, 0, -1), 5.0, (0.5, 0.0)),
    'edge bc': ((1, 3, 1), (0, 0, -1), 1.0, (0.25, 0.75)),
    'edge ca': ((0, 1, 2), (0, 0, -2), 1.0, (0.0, 0.25)),
    'vertex a': ((0, 0, 1), (0, 0, -1), 1.0, (0.0, 0.0)),
    'vertex b': ((4, 0, 1), (0, 0, -1), 1.0, (1.0, 0.0)),
    'vertex c': ((0, 4, 1), (0, 0, -1), 1.0, (0.0, 1.0)),
    'along x onto the plane x = const': ((-3, 1, 0), (1, 0, 0), None, None),     # in the plane of the face: det == 0
}


@pytest.mark.parametrize('side', [1, -1])
@pytest.mark.parametrize('name', list(HITS))
def test_one_triangle_by_hand_from_both_sides(name, side):
    o, d, t, bary = HITS[name]
    o, d = (o[0], o[1], side * o[2]), (d[0], d[1], side * d[2])
    face, t32, b, t64 = one(o, d)
    if t is None:
        assert face == -1 and t32 == INF and np.isnan(b).all()
        return
    assert face == 0 and t64 == t and t32 == t and b == list(bary)


def test_misses_and_rays_parallel_to_the_plane():
    for o, d in (((5, 5, 1), (0, 0, -1)), ((-0.5, 1, 1), (0, 0, -1)), ((1, 1, 1), (0, 0, 1)),      # beside it; pointing away
                 ((1, 1, 1), (1, 0, 0)), ((1, 1, 1), (-1, 2, 0)), ((1, 1, 0), (1, 1, 0))):          # parallel, above and within
        face, t, b, t64 = one(o, d)
        assert face == -1 and t == INF and t64 == INF and np.isnan(b).all(), (o, d)


def test_t_exactly_at_tmin_and_at_tmax_counts():
    o, d = (1, 1, 3), (0, 0, -1)
    assert one(o, d, 3.0, 3.0)[:2] == (0, 3.0)
    assert one(o, d, 0.0, 3.0)[0] == 0 and one(o, d, 3.0, INF)[0] == 0
    below, above = float(np.nextafter(F32(3), F32(0))), float(np.nextafter(F32(3), F32(4)))
    assert one(o, d, 0.0, below)[:2] == (-1, INF) and one(o, d, above, INF)[:2] == (-1, INF)
    assert one((1, 1, -3), d, -5.0, 0.0)[:2] == (0, -3.0)                                   # a negative parameter is a parameter
    assert one((1, 1, -3), d)[0] == -1


@pytest.mark.parametrize('bad', [
    dict(o=(np.nan, 0, 0)), dict(o=(0, INF, 0)), dict(o=(0, 0, -INF)), dict(d=(np.nan, 0, -1)), dict(d=(0, INF, -1)),
    dict(d=(0, 0, -INF)), dict(d=(0, 0, 0)), dict(tmin=np.nan), dict(tmin=INF), dict(tmin=-INF), dict(tmax=np.nan),
    dict(tmin=2.0, tmax=1.0), dict(tmax=-INF)])
def test_every_kind_of_invalid_ray(bad):
    args = dict(o=(1, 1, 3), d=(0, 0, -1), tmin=0.0, tmax=INF)
    assert one(**args)[0] == 0
    args.update(bad)
    face, t, b, t64 = one(**args)
    assert face == -1 and np.isnan(t) and np.isnan(t64) and np.isnan(b).all()


def test_tmax_infinite_and_negative_zero_direction_components_are_valid():
    assert one((1, 1, 3), (-0.0, 0.0, -1), 0.0, INF)[:2] == (0, 3.0)
    assert one((1, 1, 3), (0, 0, -1), 3.0, 3.0)[0] == 0                                      # tmax == tmin is an interval


def test_zero_area_faces_are_never_hit():
    v = np.asarray([[0, 0, 0], [1, 0, 0], [2, 0, 0], [1, 1, 1]], F32)
    for f in ([0, 1, 2], [0, 1, 0], [3, 3, 3], [0, 0, 2]):                                  # a line, a repeated vertex, a point
        for o, d in (((1, 0, 1), (0, 0, -1)), ((1, 1, 2), (0, 0, -1)), ((0.5, 0, 3), (0, 0, -1)), ((-1, 0, 0), (1, 0, 0))):
            assert one(o, d, verts=v, faces=np.asarray([f], I32))[0] == -1, (f, o, d)


def test_skip_removes_exactly_the_skipped_face():
    v = np.concatenate([TRI_V, TRI_V + F32([0, 0, -1]), TRI_V + F32([0, 0, -2])])
    f = np.asarray([[0, 1, 2], [3, 4, 5], [6, 7, 8]], I32)
    o, d = (1, 1, 3), (0, 0, -1)
    assert one(o, d, verts=v, faces=f)[:2] == (0, 3.0)
    assert one(o, d, verts=v, faces=f, skip=0)[:2] == (1, 4.0)
    assert one(o, d, verts=v, faces=f, skip=1)[:2] == (0, 3.0)
    assert one(o, d, verts=v, faces=f, skip=-1)[:2] == (0, 3.0)
    assert one(o, d, verts=v[:3], faces=f[:1], skip=0)[:2] == (-1, INF)


def test_two_faces_at_equal_t_give_the_lower_index():
    v = np.asarray([[0, 0, 0], [4, 0, 0], [4, 4, 0], [0, 4, 0], [0, 0, 1], [4, 0, 1], [0, 4, 1]], F32)
    quad = [[0, 1, 2], [0, 2, 3]]                                                          # the diagonal (0,0,0) - (4,4,0) is shared
    for faces, want in ((quad, 0), (quad[::-1], 0), ([[4, 5, 6]] + quad, 0), (quad + quad, 0), ([quad[1], quad[1], quad[0]], 0)):
        face, t, _, _ = one((2, 2, 5), (0, 0, -1), verts=v, faces=np.asarray(faces, I32))
        assert (face, t) == (want, 4.0 if len(faces) == 3 and faces[0] == [4, 5, 6] else 5.0), faces
    face = one((2, 2, 5), (0, 0, -1), verts=v, faces=np.asarray(quad + quad, I32), skip=0)[0]
    assert face == 1                                                                       # then the next lowest at the same t


@pytest.fixture(scope='module')
def sphere1280():
    v, f = C.icosphere(3)
    assert v.shape == (642, 3) and f.shape == (1280, 3)
    return v, f


def _edge_points(v, f):
    e = np.unique(np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), 1), axis=0)
    assert len(e) == 1920
    w = np.arange(1, 7, dtype=F64) / 7.0
    a, b = v[e[:, 0]].astype(F64), v[e[:, 1]].astype(F64)
    return (a[:, None] * (1 - w)[None, :, None] + b[:, None] * w[None, :, None]).reshape(-1, 3)


def test_no_ray_through_a_vertex_or_an_edge_slips_between_faces(sphere1280):
    """The issue's figures: from the centre exactly through the 642 vertices, and from an off-centre point through the vertices
    and six points on every edge (12,162 rays), the watertight rule misses nothing; plain fp64 Moller-Trumbore does."""
    v, f = sphere1280
    zero = np.zeros((len(v), 3), F32)
    face, t, _, _ = C.cast_rays(zero, v, 0.0, INF, v, f)                                # d = the vertex itself: exactly through it
    assert np.all(face >= 0) and np.all(np.abs(t - 1) < 1e-6)
    naive = C.moller_trumbore_hits(zero, v, v, f)
    assert naive.sum() < len(v), 'the naive test is expected to lose rays here: that is what the watertight rule is for'
    print('Moller-Trumbore finds', int(naive.sum()), 'of', len(v))
    o = np.asarray([0.3, -0.2, 0.1], F32)
    targets = np.concatenate([v.astype(F64), _edge_points(v, f)])
    assert len(targets) == 12162
    d = (targets - o.astype(F64)).astype(F32)
    face, t, _, _ = C.cast_rays(np.broadcast_to(o, d.shape), d, 0.0, INF, v, f)
    assert int((face < 0).sum()) == 0
    assert np.all(np.abs(t - 1) < 1e-3)                                                    # the far side is at t ~ 1


def test_the_fibonacci_set():
    from mvip_nerf_amd import mesh
    for K in (1, 16, 32, 255):
        d = C.fibonacci_directions(K)
        assert d.dtype == F32 and d.shape == (K, 3)
        np.testing.assert_array_equal(mesh.fibonacci_directions(K), d)
        np.testing.assert_allclose(np.linalg.norm(d.astype(F64), axis=1), 1.0, atol=1e-6)
        want_z = [1.0 - (2 * i + 1) / K for i in range(K)]
        np.testing.assert_array_equal(d[:, 2], np.asarray(want_z, F64).astype(F32))
        for i in (0, K // 2, K - 1):
            phi, r = math.pi * (1 + math.sqrt(5)) * (i + 0.5), math.sqrt(1 - want_z[i] ** 2)
            assert abs(d[i, 0] - r * math.cos(phi)) < 1e-6 and abs(d[i, 1] - r * math.sin(phi)) < 1e-6
    d = C.fibonacci_directions(32).astype(F64)
    assert np.abs(d.mean(0)).max() < 0.02                                                   # balanced
    gram = d @ d.T - 2 * np.eye(32)
    assert gram.max() < math.cos(math.radians(25))                                          # and spread: no two within 25 degrees
    for bad in (0, 256, 1.5, True):
        with pytest.raises(ValueError, match='count'):
            mesh.fibonacci_directions(bad)


@pytest.mark.parametrize('level,K', [(2, 16), (1, 16), (2, 64)])
def test_nested_spheres_openness(level, K):
    v, f, n_outer = C.nested_spheres(level)
    assert n_outer == 20 * 4 ** level and len(f) == 2 * n_outer
    fo, ft, bo, bt = C.face_openness(v, f, C.fibonacci_directions(K))
    assert np.all(ft + bt == K)                                                            # no direction had N . d == 0
    assert ft.min() >= 6 and bt.min() >= 6
    outer, inner = slice(0, n_outer), slice(n_outer, None)
    assert np.array_equal(fo[outer], ft[outer]) and np.all(bo[outer] == 0)
    assert np.all(fo[inner] == 0) and np.all(bo[inner] == 0)
    # within reach of nothing every direction is open: the inner sphere is 0.5 away from the outer one at the nearest
    fo, ft, bo, bt = C.face_openness(v, f, C.fibonacci_directions(K), max_dist=0.01)
    assert np.array_equal(fo[outer], ft[outer]) and np.array_equal(fo[inner], ft[inner])


def test_lattice_mesh_and_rays_are_what_the_gpu_test_needs():
    v, f = C.lattice_mesh()
    assert f.shape == (64, 3) and np.all(v == np.round(v)) and v.min() == 0 and v.max() == 4
    o, d, tmin, tmax = C.lattice_rays()
    assert 1200 <= len(o) <= 1400 and len(o) % 64 != 0
    assert C.valid_rays(o, d, tmin, tmax).all()
    in_plane = ((d == 0) & (o == np.round(o))).any(1)
    assert in_plane.sum() > 200
    face = C.cast_rays(o, d, tmin, tmax, v, f)[0]
    assert 0.25 < (face >= 0).mean() < 0.9 and len(np.unique(face)) > 40


NEW_SYMBOLS = ('mvip_mesh_raycast', 'mvip_mesh_face_openness')


def test_header_and_binding_table_hold_the_new_symbols():
    from mvip_nerf_amd import _lib
    from mvip_nerf_amd.csrc.build import SOURCES
    import test_abi
    assert 'mesh_raycast.hip' in SOURCES
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
    bounds = (ctypes.c_float * 6)(0, 0, 0, 2, 2, 2)
    nanbounds = (ctypes.c_float * 6)(0, 0, 0, 2, float('inf'), 2)
    flipped = (ctypes.c_float * 6)(0, 3, 0, 2, 2, 2)
    one, null, st = 16, None, None                        # a non-NULL pointer that is never dereferenced: every call below is refused
    INT = 2 ** 31 - 1
    cast = lambda **k: lib.mvip_mesh_raycast(*[k.get(n, d) for n, d in (
        ('o', one), ('d', one), ('tmin', null), ('tmax', null), ('tmin_all', 0.0), ('tmax_all', 1.0), ('skip', null), ('N', 2),
        ('verts', one), ('faces', one), ('V', 3), ('F', 1), ('box', box), ('cells', cells), ('bounds', bounds), ('coff', one),
        ('cfaces', one), ('P', 4), ('any', 0), ('face', one), ('t', one), ('bary', null), ('stats', null))], st)
    for bad in (dict(F=0), dict(V=0), dict(F=-1), dict(F=INT), dict(V=INT + 1), dict(N=-1), dict(N=INT), dict(P=-1), dict(P=INT + 1),
                dict(box=nanbox), dict(box=zinv), dict(box=None), dict(cells=big), dict(cells=None), dict(bounds=None),
                dict(bounds=nanbounds), dict(bounds=flipped), dict(any=2), dict(any=-1), dict(o=null), dict(d=null), dict(verts=null),
                dict(faces=null), dict(coff=null), dict(cfaces=null), dict(face=null)):
        assert cast(**bad) == -1, bad
    openness = lambda **k: lib.mvip_mesh_face_openness(*[k.get(n, d) for n, d in (
        ('verts', one), ('faces', one), ('V', 3), ('F', 1), ('box', box), ('cells', cells), ('bounds', bounds), ('coff', one),
        ('cfaces', one), ('P', 4), ('dirs', one), ('K', 16), ('max_dist', float('inf')), ('counts', one), ('stats', null))], st)
    for bad in (dict(F=0), dict(V=0), dict(F=INT // 4 + 1), dict(P=-1), dict(box=nanbox), dict(cells=big), dict(bounds=None),
                dict(bounds=flipped), dict(K=-1), dict(K=256), dict(max_dist=float('nan')), dict(max_dist=-1.0), dict(dirs=null),
                dict(counts=null), dict(verts=null), dict(faces=null), dict(coff=null), dict(cfaces=null)):
        assert openness(**bad) == -1, bad
