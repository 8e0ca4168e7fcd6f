"""The signed mesh distance's restatement (tests/mesh_sdf_numpy.py) against analytic facts, without a GPU: the sign of the
angle-weighted pseudonormal equals the half-space inside test of convex meshes on every query, the two cheaper signs it replaces
do not, and every feature code occurs.  tests/test_mesh_sdf.py holds the kernels to this restatement bit for bit."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_distance_numpy as D                          # noqa: E402
import mesh_sdf_numpy as S                               # noqa: E402

F32 = np.float32
N_POINTS = 4000
# mesh -> (builder, box lo, box hi) of the seed-0 uniform queries
CONVEX = {
    'tetrahedron': (S.tetrahedron, (-0.75, -0.75, -0.75), (0.75, 0.75, 0.75)),
    'spike': (S.spike, (-0.15, -0.15, -0.1), (0.15, 0.15, 1.1)),
    'fan_spike': (S.fan_spike, (-0.1, -0.1, 0.85), (0.1, 0.1, 1.15)),          # about the apex, where the slivers meet
    'fan_spike_whole': (S.fan_spike, (-0.15, -0.15, -0.1), (0.15, 0.15, 1.1)),  # the whole of it: the apex box holds few inside points
    'cube': (lambda: D.cube_mesh(0.5), (-0.75, -0.75, -0.75), (0.75, 0.75, 0.75)),
}
_cache = {}


def convex_case(name):
    """(verts, faces, points, closest_feature(...), inside) made once and left unchanged"""
    if name not in _cache:
        build, lo, hi = CONVEX[name]
        v, f = build()
        pts = np.random.default_rng(0).uniform(lo, hi, (N_POINTS, 3)).astype(F32)
        closest = S.closest_feature(pts, v, f)
        inside, margin = S.convex_inside(pts, v, f)
        assert margin.min() > 1e-6                           # no query sits on a face plane: the analytic answer is not in doubt
        for a in (v, f, pts, inside) + closest:
            a.setflags(write=False)
        _cache[name] = (v, f, pts, closest, inside)
    return _cache[name]


def wrong_signs(name, **kw):
    v, f, pts, closest, inside = convex_case(name)
    sd = S.signed_distance(pts, v, f, closest=closest, **kw)[0]
    assert np.all(np.isfinite(sd)) and np.all(sd != 0)       # nothing left out
    return int(np.sum((sd < 0) != inside)), int(inside.sum())


def test_meshes_are_what_the_names_say():
    import mesh_topology_numpy as T
    for name, faces in (('tetrahedron', 4), ('spike', 4), ('fan_spike', 34), ('fan_spike_whole', 34), ('cube', 12)):
        v, f = CONVEX[name][0]()
        assert len(f) == faces
        r = T.report(f, len(v))
        assert r['closed'] and r['oriented'] and r['components'] == 1 and r['genus'] == 0, (name, r)


@pytest.mark.parametrize('name', list(CONVEX))
def test_pseudonormal_sign_equals_the_analytic_inside_test(name):
    wrong, n_inside = wrong_signs(name)
    print(name, 'wrong signs', wrong, 'of', N_POINTS, 'inside', n_inside)
    assert 0 < n_inside < N_POINTS
    assert wrong == 0


def test_face_normal_sign_fails_on_the_tetrahedron():
    wrong, _ = wrong_signs('tetrahedron', mode='face')
    print('face-normal sign: wrong', wrong, 'of', N_POINTS)
    assert wrong > 0


def test_unweighted_vertex_sum_fails_at_the_fan_spike_apex():
    v, f = convex_case('fan_spike')[:2]
    wrong, _ = wrong_signs('fan_spike', P=S.vertex_pseudonormals(v, f, weighted=False))
    print('unweighted vertex sum: wrong', wrong, 'of', N_POINTS)
    assert wrong > 0


def test_every_feature_code_occurs_on_the_tetrahedron():
    feat = convex_case('tetrahedron')[3][3]
    assert sorted(np.unique(feat).tolist()) == [0, 1, 2, 3, 4, 5, 6]


def test_feature_codes_name_the_feature_that_holds_q():
    v, f, pts, (face, q, d2, feat), _ = convex_case('tetrahedron')
    vv = v.astype(np.float64)
    tri = vv[f[face]]                                        # [N, 3, 3]
    for k in range(3):
        at = feat == 4 + k
        assert at.any() and np.array_equal(q[at], tri[at, k])              # a vertex code: q IS that vertex
        on = feat == 1 + k
        a, b = tri[on, k], tri[on, (k + 1) % 3]
        t = D._dot(q[on] - a, b - a) / D._dot(b - a, b - a)
        assert on.any() and np.all((t > 0) & (t < 1))
        assert np.abs(np.cross(q[on] - a, b - a)).max() < 1e-12            # an edge code: q on that edge's line


def test_the_pruned_reference_equals_brute_force():
    import mesh_raycast_numpy as C
    v, f = C.icosphere(2, 0.8)
    pts = S.query_set(v, f, 500, 1)
    brute, pruned = S.closest_feature(pts, v, f), S.closest_feature(pts, v, f, prune=True)
    for x, y in zip(brute, pruned):
        np.testing.assert_array_equal(x, y)
    v, f = S.open_degenerate()
    pts = S.query_set(v, f, 500, 2)
    for x, y in zip(S.closest_feature(pts, v, f), S.closest_feature(pts, v, f, prune=True)):
        np.testing.assert_array_equal(x, y)
